"""CPU-only: fsh_view_exact_axes (the axes the exact renderer reads) against Python Fraction floors of the same bounding-box
strings, every column and row, centre axis and both shifted axes at three ladder levels."""
from fractions import Fraction

import numpy as np
import pytest

import _truth
from fractalshark_amd import exact, inputs

CASES = [("view0_70x37", 187), ("shallow_1e-28", None), ("x2_c1_1e-40", None), ("view19_64x36", 707)]
LEVELS = (10, 22, 35)


def _view(name):
    if name == "view19_64x36":
        return inputs.View.builtin(19, 64, 36, antialiasing=1), 64, 36
    c = _truth.Case(name)
    return c.view(inputs), c.w, c.h


def _value(planes, i):
    """Column / row i of a limb-major axis as a signed Python integer."""
    L = planes.shape[0]
    v = sum(int(planes[l, i]) << (32 * l) for l in range(L))
    return v - (1 << (32 * L)) if v >> (32 * L - 1) else v


@pytest.mark.parametrize("name,F", CASES)
def test_axes_equal_fraction_floors(native_libs, name, F):
    v, w, h = _view(name)
    F = _truth.fixture()["cases"][name]["frac_bits"] if F is None else F
    assert F == v.precision_bits + _truth.GUARD_BITS
    bbox = v.bbox()
    if name == "x2_c1_1e-40":
        assert any(s.startswith("-") and "e-41" in s for s in bbox), bbox  # negative, tiny: the strings the parser must read
    minx, miny, maxx, maxy = (Fraction(s) for s in bbox)
    fix = lambda q: (q.numerator << F) // q.denominator
    L = exact.limbs_for(F)
    assert L == -(-(F + 10) // 32)
    cx, cy = exact.axes(v, F)
    assert cx.shape == (L, w) and cy.shape == (L, h) and cx.dtype == np.uint32
    want_x = [minx + (maxx - minx) * x / w for x in range(w)]
    want_y = [maxy - (maxy - miny) * y / h for y in range(h)]
    assert [_value(cx, x) for x in range(w)] == [fix(q) for q in want_x]
    assert [_value(cy, y) for y in range(h)] == [fix(q) for q in want_y]
    for level in LEVELS:
        s = (maxx - minx) / (1 << level)
        cx3, cy3 = exact.axes(v, F, level=level)
        assert cx3.shape == (3, L, w) and cy3.shape == (3, L, h)
        for k, d in enumerate((0, s, -s)):
            assert [_value(cx3[k], x) for x in range(w)] == [fix(q + d) for q in want_x], (level, k)
            assert [_value(cy3[k], y) for y in range(h)] == [fix(q + d) for q in want_y], (level, k)


def test_axes_refuse_what_does_not_fit(native_libs):
    v = inputs.View.builtin(0, 70, 37)
    with pytest.raises(ValueError):
        exact.axes(v, 187, limbs=5)  # |c| ~ 2 needs 187 + 3 bits
    cx, _ = exact.axes(v, 187, limbs=8)  # more limbs than needed: sign-extended
    cx7, _ = exact.axes(v, 187, limbs=7)
    assert [_value(cx, x) for x in range(70)] == [_value(cx7, x) for x in range(70)]
