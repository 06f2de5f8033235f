"""CPU-only: the parts of the wide exact kernel that need no wave (csrc/exact_wide_math.hpp), built for the host with g++
(tests/exact/exact_wide_host.cpp, 64 lanes in a loop) and compared with Python integers: the carry look-ahead, the 64-block
addition made of it, the block-wise bailout compare.  Then the axes at View 14's 683 limbs, the constants and the dispatch rule."""
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
SRC = os.path.join(HERE, "exact", "exact_wide_host.cpp")
HDRS = [os.path.join(os.path.dirname(HERE), "fractalshark_amd", "csrc", f) for f in ("exact_wide_math.hpp", "exact_math.hpp")]
SO = os.path.join(HERE, "exact", "libexact_wide_host.so")
FULL = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or max(os.path.getmtime(p) for p in [SRC] + HDRS) > os.path.getmtime(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC], check=True)
    h = C.CDLL(SO)
    h.exw_carry_in_mask.restype = C.c_uint64
    h.exw_carry_in_mask.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]
    return h


def _block_sizes(lib):
    out = (C.c_uint32 * 32)()
    return list(out[:lib.exw_block_sizes(out, 32)])


def _arr(v, n):
    v &= (1 << (32 * n)) - 1
    return (C.c_uint32 * n)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)])


def _int(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def _ripple(G, P, cin):
    """The carry into every block, one block after the other."""
    mask, c = 0, cin
    for t in range(64):
        mask |= c << t
        g, p = (G >> t) & 1, (P >> t) & 1
        c = 1 if g else (c if p else 0)
    return mask, c


def _look_ahead(lib, G, P, cin):
    cout = C.c_uint32(7)
    return lib.exw_carry_in_mask(G, P, cin, C.byref(cout)), cout.value


def test_block_sizes_and_constants(lib):
    assert _block_sizes(lib) == list(range(1, 12))
    assert lib.exw_max_limbs() == exact.MAX_WIDE_LIMBS == 704 == 64 * 11
    assert exact.MAX_WIDE_FRAC_BITS == 22518 == 32 * 704 - 10
    assert (exact.MIN_LIMBS, exact.MAX_LIMBS, exact.MAX_FRAC_BITS) == (2, 24, 758)
    assert [lib.exw_block_for(L) for L in (2, 64, 65, 128, 129, 683, 704)] == [1, 1, 2, 2, 3, 11, 11]
    assert exact.limbs_for(21829) == 683 and exact.limbs_for(22518) == 704 and exact.limbs_for(2550) == 80
    assert lib.exw_add(12, None, None, 0, None) == -1 and lib.exw_add(0, None, None, 0, None) == -1


def test_dispatch_rule_of_render():
    """Frames that render today take the path they take today; the wide kernel starts where the narrow one ends."""
    assert not exact.uses_wide(exact.limbs_for(758)) and exact.uses_wide(exact.limbs_for(759))
    assert [exact.uses_wide(L) for L in (2, 23, 24, 25, 704)] == [False, False, False, True, True]

    class Spy:
        def __init__(self):
            self.calls = []

        def RenderExact(self, *a):
            self.calls.append(("narrow", a[2]))
            return 0

        def RenderExactWide(self, *a):
            self.calls.append(("wide", a[2]))
            return 0

    spy = Spy()
    v = inputs.View.builtin(0, 8, 4, antialiasing=1)
    for F in (187, 758, 759, 2550):
        exact.render(spy, v, frac_bits=F)
    assert spy.calls == [("narrow", 7), ("narrow", 24), ("wide", 25), ("wide", 80)]


def test_carry_look_ahead_equals_the_ripple(lib):
    rng = random.Random(11)
    cases = [(0, 0), (FULL, 0), (0, FULL), (1, FULL ^ 1), (1 << 63, 0), (0, 1 << 63)]
    for _ in range(4000):
        G = rng.getrandbits(64) & rng.getrandbits(64)
        P = rng.getrandbits(64) & ~G
        cases.append((G, P))
    for _ in range(500):  # dense propagate masks: long runs
        G = rng.getrandbits(64) & rng.getrandbits(64) & rng.getrandbits(64)
        cases.append((G, FULL & ~G & (rng.getrandbits(64) | rng.getrandbits(64) | rng.getrandbits(64))))
    for run in range(1, 65):  # all-propagate runs of 1 .. 64 blocks, at every place, fed by carry-in or by a generate below
        for start in sorted({0, 1, 64 - run, rng.randrange(0, 65 - run)}):
            P = ((1 << run) - 1) << start
            cases.append((0, P))
            if start:
                cases.append((1 << (start - 1), P))
    for G, P in cases:
        for cin in (0, 1):
            assert _look_ahead(lib, G, P, cin) == _ripple(G, P, cin), (hex(G), hex(P), cin)
    # a block cannot generate and propagate; where a caller says both, generate wins
    assert _look_ahead(lib, 1, 3, 0) == _ripple(1, 2, 0)


@pytest.mark.parametrize("M", [1, 2, 3, 11])
def test_64_block_addition_equals_python(lib, M):
    rng = random.Random(12 + M)
    n = 64 * M
    full = (1 << (32 * n)) - 1
    blk = (1 << (32 * M)) - 1
    pairs = [(0, 0), (full, 0), (full, 1), (full, full), (1, full - 1), (full >> 1, 1), (1 << (32 * n - 1), 1 << (32 * n - 1))]
    for run in range(1, 65):  # `run` blocks of ones above a block that overflows into them, and the same with nothing coming in
        start = rng.randrange(0, 65 - run)
        ones = (((1 << (32 * M * run)) - 1) << (32 * M * start)) & full
        below = (blk << (32 * M * (start - 1))) if start else 0
        pairs += [(ones | below, (1 << (32 * M * (start - 1))) if start else 0), (ones, 0), (ones, rng.getrandbits(32 * n) & ~ones & full)]
    pairs += [(rng.getrandbits(32 * n), rng.getrandbits(32 * n)) for _ in range(40)]
    pairs += [(v, full ^ v) for v in (rng.getrandbits(32 * n) for _ in range(10))]  # a + ~a: every block all ones
    out = (C.c_uint32 * n)()
    for a, b in pairs:
        for cin in (0, 1):
            cout = lib.exw_add(M, _arr(a, n), _arr(b, n), cin, out)
            s = a + b + cin
            assert (_int(out), cout) == (s & full, s >> (32 * n)), (M, hex(a)[:40], hex(b)[:40], cin)


@pytest.mark.parametrize("M", [1, 2, 3, 11])
def test_block_wise_bailout_compare_equals_python(lib, M):
    rng = random.Random(20 + M)
    n = 128 * M
    for L in sorted({2 if M == 1 else 64 * (M - 1) + 1, 64 * M - 3, 64 * M}):
        fmax = 32 * L - 10
        for F in sorted({fmax, fmax - 5, 32 * (L - 1), 16 * L, 16 * M, 32 * M, 17} & set(range(1, fmax + 1))):
            for R in (1, 4, 255, 256):
                bail = R << (2 * F)
                for s in (0, bail, bail - 1, bail + 1, bail + (1 << 32), bail - (1 << 32), bail << 1, bail >> 1, bail + (1 << (32 * M)),
                          bail - (1 << (32 * M)) if bail >> (32 * M) else 1, 1 << (32 * n - 1), rng.getrandbits(2 * F + 10),
                          rng.getrandbits(32 * n)):
                    for inclusive in (0, 1):
                        want = 1 if (s > bail or (inclusive and s == bail)) else 0
                        assert lib.exw_exceeds(M, _arr(s, n), F, R, inclusive) == want, (M, L, F, R, s - bail, inclusive)


def _fraction(text):
    """Fraction(text) for a decimal string of any length (Python refuses to read more than 4300 digits into an int in one go)."""
    t = text.strip().lower()
    mant, _, exp = t.partition("e")
    neg = mant.startswith("-")
    whole, _, frac = mant.lstrip("+-").partition(".")
    digits, n = whole + frac, 0
    for i in range(0, len(digits), 4000):
        chunk = digits[i:i + 4000]
        n = n * 10 ** len(chunk) + int(chunk)
    q = Fraction(-n if neg else n) * Fraction(10) ** (int(exp or 0) - len(frac))
    return q


def test_axes_at_683_limbs_equal_fraction_floors(native_libs):
    """View 14 at the fixture's 21 829 fractional bits, as a 16 x 9 frame: a few columns and rows, and one ladder level."""
    w, h = 16, 9
    v, F = inputs.View.builtin(14, w, h, antialiasing=1), _truth.fixture()["cases"]["view14_15360x8640_attempt"]["frac_bits"]
    assert F == 21829 == v.precision_bits + _truth.GUARD_BITS and exact.limbs_for(F) == 683
    assert _fraction("-12.5e-1") == Fraction(-5, 4)
    minx, miny, maxx, maxy = (_fraction(s) for s in v.bbox())
    fix = lambda q: (q.numerator << F) // q.denominator
    val = lambda planes, i: (lambda u: u - (1 << (32 * 683)) if u >> (32 * 683 - 1) else u)(_int(planes[:, i]))
    cx, cy = exact.axes(v, F)
    assert cx.shape == (683, w) and cy.shape == (683, h)
    for x in (0, 1, 7, w - 1):
        assert val(cx, x) == fix(minx + (maxx - minx) * x / w), x
    for y in (0, 4, h - 1):
        assert val(cy, y) == fix(maxy - (maxy - miny) * y / h), y
    s = (maxx - minx) / (1 << 35)
    cx3, cy3 = exact.axes(v, F, level=35)
    for k, d in enumerate((0, s, -s)):
        assert val(cx3[k], 7) == fix(minx + (maxx - minx) * 7 / w + d)
        assert val(cy3[k], 4) == fix(maxy - (maxy - miny) * 4 / h + d)
