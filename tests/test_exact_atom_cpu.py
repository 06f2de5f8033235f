"""CPU-only: csrc/exact_atom_math.hpp -- the exact renderer's step loop with the period planes' rule -- built for the host with g++
(tests/exact/exact_atom_host.cpp) against the definitions restated on Python integers (tests/_atom_model.py): the value v of every
sample, its atom period A, the index it was proved at, its cycle length, and how often the smallest norm was read back with the
narrowest key the header allows."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _atom_model as model
import _cycle_model as cycle
from fractalshark_amd import exact

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "exact", "exact_atom_host.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "fractalshark_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("exact_atom_math.hpp", "exact_cycle_math.hpp", "exact_math.hpp")]
SO = os.path.join(HERE, "exact", "libexact_atom_host.so")

# frac_bits of 2, 8 and 24 limbs, the largest each holds
FS = (54, 246, 758)
NARROWEST = 6  # key bits: the index of the highest limb that is not zero, alone


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or max(os.path.getmtime(p) for p in [SRC] + HDRS) > os.path.getmtime(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC, "-lpthread"], check=True)
    h = C.CDLL(SO)
    h.exa_atom_runs.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_int,
                                C.c_uint32, C.c_void_p, C.c_int]
    h.exa_atom_key8.restype = C.c_uint64
    h.exa_atom_key8.argtypes = [C.c_void_p, C.c_uint32]
    return h


def _limbs(v, L):
    v &= (1 << (32 * L)) - 1
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(L)]


def _host(lib, cxs, cys, F, R, inclusive, cap, check, key_bits=0):
    """The header's loop on the samples (Python integers): int64[n, 7] = outcome, value, atom, proof index, cycle length, steps,
    read-backs of the minimum."""
    L, n = exact.limbs_for(F), len(cxs)
    cx = np.array([_limbs(v, L) for v in cxs], np.uint32)
    cy = np.array([_limbs(v, L) for v in cys], np.uint32)
    out = np.zeros((n, 7), np.uint64)
    assert lib.exa_atom_runs(L, n, cx.ctypes.data, cy.ctypes.data, F, R, 1 if inclusive else 0, cap, 1 if check else 0, key_bits,
                             out.ctypes.data, 16) == 0
    return out.astype(np.int64)


def _fix(c, F):
    return tuple((Fraction(v).numerator << F) // Fraction(v).denominator for v in c)


def _both(lib, c, F, cap, R=4, inclusive=False):
    """One sample c (a pair of Fractions): the model's (v, A, proof index, cycle length) after the host loop has been found equal to
    it, with the cycle check off and on, with the full key and the narrowest (which must change nothing but the read-backs, and
    those must be the model's)."""
    cx, cy = _fix(c, F)
    off = model.sample(cx, cy, F, R, inclusive, cap, check=False)
    on = model.sample(cx, cy, F, R, inclusive, cap, check=True)
    assert off[:4] == on[:4], (c, F, cap)
    for check, m in ((False, off), (True, on)):
        for bits in (0, 32, NARROWEST):
            got = _host(lib, [cx], [cy], F, R, inclusive, cap, check, bits)[0]
            assert int(got[1]) == m[0] and int(got[2]) == m[1], (c, F, cap, R, inclusive, check, bits, got, m)
            assert (int(got[3]), int(got[4])) == ((m[2], m[3]) if check else (0, 0)), (c, F, cap, check, bits, got, m)
            if bits == NARROWEST:
                assert int(got[6]) == m[4], (c, F, cap, check, got, m)
            elif bits == 0:
                assert int(got[6]) <= m[4]
    return off[:4]


def test_the_key_is_monotone(lib):
    """key(a) <= key(b) for a <= b over 8-limb numbers of every size, with zero top limbs, at every width the hook allows; numbers that
    differ in the 58 bits the full key holds below its limb index get different keys."""
    rng = np.random.default_rng(5)
    vals = {0, 1, 2, (1 << 256) - 1}
    for bits in range(1, 257, 5):
        for _ in range(6):
            v = int(rng.integers(0, 1 << 62)) << max(0, bits - 62) if bits > 62 else int(rng.integers(0, 1 << bits))
            v &= (1 << bits) - 1
            vals.update((v, v | (1 << (bits - 1)), (v | (1 << (bits - 1))) + 1 if bits < 256 else v))
    vals = sorted(v for v in vals if v < 1 << 256)

    def key(v, kb):
        a = np.array(_limbs(v, 8), np.uint32)
        return int(lib.exa_atom_key8(a.ctypes.data, kb))

    for kb in (0, 40, NARROWEST, 3):
        keys = [key(v, kb) for v in vals]
        assert all(a <= b for a, b in zip(keys, keys[1:])), kb
    assert [key(v, NARROWEST) for v in (0, 1, 1 << 32, (1 << 64) - 1, 1 << 224)] == [0, 0, 1, 1, 7]
    assert key(3, 3) == key(3, NARROWEST)  # (below 6 bits: 6)
    assert key(1 << 64, 0) < key((1 << 64) + (1 << 38), 0) and key(5, 0) < key(6, 0)


@pytest.mark.parametrize("F", FS)
def test_zero_and_minus_one(lib, F):
    assert exact.limbs_for(F) in (2, 8, 24)
    # c = 0: every norm is 0, the earliest stays: A = 1; z_2 == z_1 is proved at n = 2 against the checkpoint of n = 1
    assert _both(lib, (0, 0), F, 1000) == (1000, 1, 2, 1)
    # c = -1: -1, 0, -1, 0: the norms repeat 1, 0, 1, 0; A = 2, and the tie at n = 4 must not replace it; proved at n = 4 against 2
    assert _both(lib, (-1, 0), F, 1000) == (1000, 2, 4, 2)
    assert _both(lib, (-1, 0), F, 1) == (1, 1, 0, 0) and _both(lib, (-1, 0), F, 2) == (2, 2, 0, 0)


@pytest.mark.parametrize("F", FS)
def test_minus_two_strict_and_inclusive(lib, F):
    # strict: -2, 2, 2, ...: all norms 4, A = 1; z_3 == z_2 proved at n = 3 against the checkpoint of n = 2
    assert _both(lib, (-2, 0), F, 1000, R=4, inclusive=False) == (1000, 1, 3, 1)
    # inclusive: z_1 escapes, nothing is tracked
    assert _both(lib, (-2, 0), F, 1000, R=4, inclusive=True) == (0, 0, 0, 0)


@pytest.mark.parametrize("F", FS)
def test_outside_parabolic_and_a_fixed_point(lib, F):
    assert _both(lib, (Fraction(5, 2), Fraction(1, 3)), F, 1000) == (0, 0, 0, 0)  # |c| > 2
    # c = 1/4 creeps up towards 1/2: the smallest norm is the first, and nothing is proved
    assert _both(lib, (Fraction(1, 4), 0), F, 3000) == (3000, 1, 0, 0)
    # c = -0.5 + 0.5i falls into an attracting fixed point: proved a few steps behind a power of two, cycle length = those few steps
    v, A, n, lam = _both(lib, (Fraction(-1, 2), Fraction(1, 2)), F, 70000 if F > 54 else 20000)
    assert n > 4096 and 0 < lam == n - (1 << ((n - 1).bit_length() - 1)) < 64 and 1 <= A < n, (F, A, n, lam)


@pytest.mark.parametrize("F", FS)
def test_near_the_period_three_nucleus(lib, F):
    """c within 1e-4 of the nucleus -0.12256 + 0.74486i: z_3 is nearly 0 and no later z comes closer before the orbit has settled on
    its cycle, whose smallest point is the one near 0 -- every third state, the first of them z_3."""
    c = (Fraction(-12256, 100000) + Fraction(3, 100000), Fraction(74486, 100000) - Fraction(2, 100000))
    v, A, n, lam = _both(lib, c, F, 3000)
    assert (v, A) == (3000, 3) and lam % 3 == 0


def test_caps_around_an_escape_and_a_proof(lib):
    """z_{cap+1} is tested, never tracked.  c = -0.75 + 0.05i escapes at some E after its smallest norm at A > 1: caps below, at
    and above A and E.  And the sample proved by its 4100th step (z_4101 == the checkpoint of 4096): its A is the full
    cap's A whether the proof comes or the cap does."""
    F = 54
    c = (Fraction(-3, 4), Fraction(1, 20))  # (escapes after a few dozen steps)
    cx, cy = _fix(c, F)
    v, A, _, _, _ = model.sample(cx, cy, F, 4, False, 1000)
    E = v + 1
    assert 10 < E < 1000 and 1 < A <= v
    for cap in (A - 1, A, A + 1, E - 2, E - 1, E, E + 1):
        got = _both(lib, c, F, cap)
        assert got[0] == min(E - 1, cap) and got[1] <= got[0]
        assert got[1] == (A if cap >= A else got[1])
    assert _both(lib, c, F, A - 1)[1] != A  # (z_A is z_{cap+1} there: tested, not tracked)
    c = (Fraction(-1, 2), Fraction(1, 2))
    full = _both(lib, c, F, 20000)
    assert full[2:] == (4101, 5)
    for cap in (4098, 4099, 4100, 4101):
        got = _both(lib, c, F, cap)
        assert got[:2] == (cap, full[1]) and got[2:] == ((4101, 5) if cap >= 4100 else (0, 0))


def test_frame_64x48(lib):
    """bbox (-2.2, -1.2) .. (1.0, 1.2) at 64 x 48, F 54, R 4, cap 20 000, cycle check off and on: the atom planes equal each other
    and the model's; the check-on run's cycle lengths equal the model's and are non-zero exactly on the proved samples."""
    w, h, F, cap = 64, 48, 54, 20000
    minx, miny, maxx, maxy = (Fraction(s) for s in ("-2.2", "-1.2", "1.0", "1.2"))
    fix = lambda q: (q.numerator << F) // q.denominator
    ax = [fix(minx + (maxx - minx) * x / w) for x in range(w)]
    ay = [fix(maxy - (maxy - miny) * y / h) for y in range(h)]
    m = model.frame(ax, ay, F, 4, False, cap, check=True)
    cyc = cycle.frame(ax, ay, F, 4, False, cap)
    assert cyc.kinds() == (2462, 580, 30)
    assert np.array_equal(m.cyclen != 0, cyc.proved) and np.array_equal(m.value, cyc.value)
    assert int((m.atom == 0).sum()) == int((m.value == 0).sum()) > 0 and bool((m.atom <= m.value).all())
    assert len(np.unique(m.atom[cyc.proved])) > 5  # (components of several periods)
    cxs, cys = ax * h, [v for v in ay for _ in range(w)]
    off = _host(lib, cxs, cys, F, 4, False, cap, False)
    on = _host(lib, cxs, cys, F, 4, False, cap, True)
    narrow = _host(lib, cxs, cys, F, 4, False, cap, True, NARROWEST)
    assert np.array_equal(off[:, 2], on[:, 2]) and np.array_equal(on[:, 2], m.atom) and np.array_equal(narrow[:, 2], m.atom)
    assert np.array_equal(off[:, 1], m.value) and np.array_equal(on[:, 1], m.value)
    assert np.array_equal(on[:, 3], m.proof_n) and np.array_equal(on[:, 4], m.cyclen) and not off[:, 3:5].any()
    assert np.array_equal(narrow[:, 6], m.readbacks) and int(m.readbacks.sum()) > 50 * w * h  # the full compare says "not less" often
    assert bool((on[:, 6] <= narrow[:, 6]).all())
    # the definition itself, without the check, on every 7th sample: the same A
    only = set(range(0, w * h, 7))
    d = model.frame(ax, ay, F, 4, False, cap, check=False, only=only)
    pick = np.array(sorted(only))
    assert np.array_equal(d.atom[pick], m.atom[pick]) and np.array_equal(d.value[pick], m.value[pick])


def test_the_recorded_model_is_the_models(native_libs):
    """tests/golden/exact_atom_model.json (what tests/test_gpu_exact_atom.py takes for the model's word on its frames): the frame at
    54 fractional bits run again whole, the others on every 13th sample."""
    import json
    import _truth
    from fractalshark_amd import inputs
    with open(model.RECORD) as f:
        fx = json.load(f)
    w, h, cap = fx["width"], fx["height"], fx["cap"]
    v = inputs.View(*fx["bbox"], w, h)
    assert (w, h, cap, len(fx["frames"])) == (64, 48, 20000, 6)
    c = _truth.Case("view0_70x37")
    cases = [(v, w, h, cap, F, R, inclusive) for F, R, inclusive in ((54, 4, False), (246, 4, False), (758, 4, False), (246, 256, False),
                                                                    (246, 4, True))]
    cases.append((c.view(inputs), c.w, c.h, c.cap, c.raw["frac_bits"], 4, False))
    for view, w, h, cap, F, R, inclusive in cases:
        cx, cy = exact.axes(view, F)
        rec = model.recorded(model.record_key(w, h, F, R, inclusive, cap), cycle.axes_crc(cx, cy))
        assert rec is not None and all(len(a) == w * h for a in rec)
        value, atom, cyclen = rec
        assert bool((cyclen != 0).any()) and bool((atom <= value).all())
        assert bool((atom == 0).any()) == (R == 4)  # (no c of these frames escapes at once under R = 256)
        only = None if F == 54 else set(range(0, w * h, 13))
        live = model.frame(cycle.from_limbs(cx), cycle.from_limbs(cy), F, R, inclusive, cap, check=True, only=only)
        pick = np.arange(w * h) if only is None else np.array(sorted(only))
        assert np.array_equal(live.value[pick], value[pick]) and np.array_equal(live.atom[pick], atom[pick])
        assert np.array_equal(live.cyclen[pick], cyclen[pick])
