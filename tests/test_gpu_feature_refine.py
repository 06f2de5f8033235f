"""features.refine_found on the GPU: found points refined to nuclei by the secant loop of exact.refine_points with
fs_exact_eval_points as its evaluator, against the same loop on Python integers (tests/_point_model.py) and its record
(tests/golden/feature_refine_vectors.json).  Equalities of integers only.  The whole View 5 fixture is tools/refine_features.py's."""
from fractions import Fraction

import pytest

import _point_model as model
from fractalshark_amd import GPURenderer, exact, features

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.close()


def _decimal(q):
    """A Fraction with a power-of-ten denominator as a decimal string."""
    digits = 40
    v = q * 10 ** digits
    assert v.denominator == 1
    s = str(abs(v.numerator)).rjust(digits + 1, "0")
    return ("-" if q < 0 else "") + s[:-digits] + "." + s[-digits:]


@pytest.mark.parametrize("F", [54, 246])
@pytest.mark.parametrize("offset", ["1e-3", "1e-5"])
def test_small_nuclei(renderer, F, offset):
    """Periods 1 .. 5 as found-point dicts next to their nuclei, the offset as their intrinsic radius: every field the model's, all
    converged, and the decimal strings are the integers exactly."""
    o = Fraction(offset)
    found = [{"cx": _decimal(Fraction(x) + o), "cy": _decimal(Fraction(y) + o / 2), "period": p, "intrinsic_radius": offset}
             for p, x, y in model.SMALL_NUCLEI]
    got = features.refine_found(renderer, found, frac_bits=F)
    assert len(got) == len(found)
    for pt, g in zip(found, got):
        c0, delta, p = model.fixture_point(pt, F)
        want = model.refine(c0, delta, p, F)
        keys = ("status", "c", "atom", "evaluations", "converged")
        assert {k: g[k] for k in keys} == {k: want[k] for k in keys}, (F, offset, p)
        assert g["log2"] == want["log2"] and g["period"] == p
        assert g["converged"] and g["atom"] == p
        assert (Fraction(g["cx"]) * (1 << F), Fraction(g["cy"]) * (1 << F)) == g["c"]


def test_fixture_point_43_equals_the_record(renderer):
    """Point 43 of the View 5 fixture (period 16 045) at F = 704, 23 limbs: status, refined c, atom period and evaluation count are
    the record's."""
    rec = model.record()
    F, q = rec["frac_bits"], rec["points"][43]
    pt = model.fixture()[43]
    assert F == 704 and exact.limbs_for(F) == 23 and pt["period"] == 16045
    g = features.refine_found(renderer, [pt], frac_bits=F, rounds=rec["rounds"])[0]
    assert (g["status"], g["c"], g["atom"], g["evaluations"], g["converged"]) == (q["status"], (int(q["cx"]), int(q["cy"])), q["atom"],
                                                                                q["evaluations"], q["converged"])
    assert g["converged"] and g["atom"] == 16045
    print("point 43 at F 704: %s after %d evaluations, log2 |z_p| %s" % (g["status"], g["evaluations"], [round(v, 1) for v in g["log2"]]))
    with pytest.raises(ValueError):
        features.refine_found(renderer, [pt], frac_bits=exact.MAX_FRAC_BITS + 1)
