"""CPU-only: csrc/exact_math.hpp -- the arithmetic of the exact renderer's kernels -- built for the host with g++
(tests/exact/exact_host.cpp) and compared with Python integers: square, product, magnitude, floor shift and the bailout compare for
every instantiated limb count, then the step loop itself against the exact-count fixture."""
import ctypes as C
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _truth
from fractalshark_amd import exact, inputs

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "exact", "exact_host.cpp")
HDR = os.path.join(os.path.dirname(HERE), "fractalshark_amd", "csrc", "exact_math.hpp")
SO = os.path.join(HERE, "exact", "libexact_host.so")
u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC, "-lpthread"], check=True)
    h = C.CDLL(SO)
    h.exh_counts.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64,
                             C.c_void_p, C.c_int]
    return h


def _limb_counts(lib):
    out = (C.c_uint32 * 64)()
    n = lib.exh_limb_counts(out, 64)
    return list(out[:n])


def _arr(v, n):
    """Python integer -> n limbs, two's complement."""
    v &= (1 << (32 * n)) - 1
    return (C.c_uint32 * n)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)])


def _int(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def _operands(L, rng):
    full = (1 << (32 * L)) - 1
    ops = [0, 1, full, 1 << (32 * L - 1), (1 << (32 * L - 1)) - 1, 0xFFFFFFFF, full ^ 0xFFFFFFFF]
    return ops + [rng.getrandbits(32 * L) for _ in range(12)] + [rng.getrandbits(32 * L - 40) for _ in range(4)]


def test_every_needed_limb_count_is_instantiated(lib):
    Ls = _limb_counts(lib)
    assert Ls == list(range(exact.MIN_LIMBS, exact.MAX_LIMBS + 1))
    assert exact.limbs_for(707) in Ls and exact.MAX_FRAC_BITS >= 707
    assert lib.exh_square(1, None, None) == -1 and lib.exh_square(exact.MAX_LIMBS + 1, None, None) == -1


def test_square_and_product_equal_python(lib):
    rng = random.Random(1)
    for L in _limb_counts(lib):
        ops = _operands(L, rng)
        p = (C.c_uint32 * (2 * L))()
        for a in ops:
            assert lib.exh_square(L, _arr(a, L), p) == 0
            assert _int(p) == a * a, (L, hex(a))
        for a in ops:
            for b in ops[:9] + ops[-3:]:
                assert lib.exh_mul(L, _arr(a, L), _arr(b, L), p) == 0
                assert _int(p) == a * b, (L, hex(a), hex(b))


def test_magnitude_equals_python(lib):
    rng = random.Random(2)
    for L in _limb_counts(lib):
        out = (C.c_uint32 * L)()
        top = 1 << (32 * L - 1)
        for v in [0, 1, -1, top - 1, -(top - 1), -(1 << 32), 1 << 32] + [rng.randrange(-top + 1, top) for _ in range(10)]:
            neg = lib.exh_magnitude(L, _arr(v, L), out)
            assert (neg, _int(out)) == (1 if v < 0 else 0, abs(v)), (L, v)


def test_floor_shift_equals_python(lib):
    """floor for either sign, zero and non-zero remainders, F a multiple of 32 and not."""
    rng = random.Random(3)
    for L in _limb_counts(lib):
        fmax = 32 * L - 10
        Fs = sorted({F for F in (fmax, fmax - 1, fmax - 9, 32 * (L - 1), 32 * (L - 1) + 1, 32 * (L - 1) - 1, 32 * (L - 2), 33, 32, 31, 1)
                     if 1 <= F <= fmax})
        out = (C.c_uint32 * L)()
        for F in Fs:
            assert any(F % 32 == 0 for F in Fs) and any(F % 32 for F in Fs)
            qmax = 1 << (32 * L - 1)  # the quotient must fit L limbs with its sign
            quotients = [0, 1, -1, qmax - 1, -qmax, rng.randrange(-qmax, qmax), rng.randrange(-qmax, qmax), rng.randrange(-1 << 40, 1 << 40)]
            for q in quotients:
                for rem in (0, 1, (1 << F) - 1, rng.randrange(1 << F)):
                    d = q * (1 << F) + rem
                    assert lib.exh_shift_floor(L, _arr(d, 2 * L), F, out) == 0
                    got = _int(out)
                    got -= (1 << (32 * L)) if got >> (32 * L - 1) else 0
                    assert got == d >> F == q, (L, F, q, rem)


def test_bailout_compare_equals_python(lib):
    rng = random.Random(4)
    for L in _limb_counts(lib):
        fmax = 32 * L - 10
        for F in sorted({fmax, fmax - 5, 32 * (L - 1), 16 * L, 17}):
            if not 1 <= F <= fmax:
                continue
            for R in (1, 4, 255, 256):
                bail = R << (2 * F)
                for s in [0, bail, bail - 1, bail + 1, bail + (1 << 32), bail - (1 << 32), bail << 1, bail >> 1, (1 << (64 * L - 1)) - 1,
                          rng.getrandbits(64 * L - 1), rng.getrandbits(2 * F + 10)]:
                    if s < 0:
                        continue
                    for inclusive in (0, 1):
                        want = 1 if (s > bail or (inclusive and s == bail)) else 0
                        assert lib.exh_exceeds(L, _arr(s, 2 * L), F, R, inclusive) == want, (L, F, R, s - bail, inclusive)


def _counts(lib, bbox, w, h, xs, ys, F, R, inclusive, limit):
    """The step loop of exact_math.hpp on the samples, c from Python Fractions (as _truth.python_exact_count makes it)."""
    minx, miny, maxx, maxy = (Fraction(s) for s in bbox)
    fix = lambda q: (q.numerator << F) // q.denominator
    L = exact.limbs_for(F)
    cx = np.array([list(_arr(fix(minx + (maxx - minx) * int(x) / w), L)) for x in xs], np.uint32)
    cy = np.array([list(_arr(fix(maxy - (maxy - miny) * int(y) / h), L)) for y in ys], np.uint32)
    out = np.zeros(len(xs), np.uint64)
    assert lib.exh_counts(L, len(xs), cx.ctypes.data, cy.ctypes.data, F, R, inclusive, limit, out.ctypes.data, 16) == 0
    return out.astype(np.int64)


@pytest.mark.parametrize("name", ["shallow_1e-20", "x2_c1_1e-40"])
def test_step_loop_reproduces_the_fixture_counts(lib, native_libs, name):
    c = _truth.Case(name)
    bbox, F = c.view(inputs).bbox(), c.raw["frac_bits"]
    for R in (4, 256):
        got = _counts(lib, bbox, c.w, c.h, c.xs, c.ys, F, R, 0, c.cap + 1)
        assert np.array_equal(got, c.counts(R)), (name, R, int((got != c.counts(R)).sum()))


def test_step_loop_on_the_boundary_samples(lib, native_libs):
    """c = 2i and c = -2: |z|^2 lands on 4 exactly; strict counts 2 and never, inclusive 1 and 1."""
    v = _truth.boundary_view(inputs)
    xs, ys = zip(*_truth.BOUNDARY_SAMPLES)
    F = v.precision_bits + _truth.GUARD_BITS
    for inclusive, want in ((0, [2, 0]), (1, [1, 1])):
        got = _counts(lib, v.bbox(), _truth.BOUNDARY_SIZE, _truth.BOUNDARY_SIZE, xs, ys, F, 4, inclusive, _truth.BOUNDARY_CAP + 1)
        assert got.tolist() == want == _truth.boundary_counts(v, bool(inclusive)).tolist()
