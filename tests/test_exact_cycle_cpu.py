"""CPU-only: csrc/exact_cycle_math.hpp -- the exact renderer's step loop with the cycle check -- built for the host with g++
(tests/exact/exact_cycle_host.cpp) against the rule restated on Python integers (tests/_cycle_model.py): the outcome of every
sample (escaped at E / capped / proved), its value, the steps it took, and how often its checkpoint was read back."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _cycle_model as model
from fractalshark_amd import exact

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "exact", "exact_cycle_host.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "fractalshark_amd", "csrc")
HDRS = [os.path.join(CSRC, "exact_cycle_math.hpp"), os.path.join(CSRC, "exact_math.hpp")]
SO = os.path.join(HERE, "exact", "libexact_cycle_host.so")

# frac_bits of 2, 8 and 24 limbs, the largest each holds
FS = (54, 246, 758)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or max(os.path.getmtime(p) for p in [SRC] + HDRS) > os.path.getmtime(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC, "-lpthread"], check=True)
    h = C.CDLL(SO)
    h.exc_cycle_runs.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64,
                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return h


def _limbs(v, L):
    v &= (1 << (32 * L)) - 1
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(L)]


def _host(lib, cxs, cys, F, R, inclusive, cap, fp_bits=0):
    """The header's loop on the samples (Python integers): (outcome, value, steps, compares), int64[n] each."""
    L, n = exact.limbs_for(F), len(cxs)
    cx = np.array([_limbs(v, L) for v in cxs], np.uint32)
    cy = np.array([_limbs(v, L) for v in cys], np.uint32)
    outcome, value = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    steps, compares = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    assert lib.exc_cycle_runs(L, n, cx.ctypes.data, cy.ctypes.data, F, R, 1 if inclusive else 0, cap, fp_bits, outcome.ctypes.data,
                              value.ctypes.data, steps.ctypes.data, compares.ctypes.data, 16) == 0
    return tuple(a.astype(np.int64) for a in (outcome, value, steps, compares))


def _both(lib, c, F, cap, R=4, inclusive=False):
    """One sample c (a pair of Fractions): the model's (outcome, value, steps) after the host loop has been found equal to it, with
    the full fingerprint and with 4 and 1 bits of it (which must change nothing but the number of compares)."""
    cx, cy = ((Fraction(v).numerator << F) // Fraction(v).denominator for v in c)
    o, v, s, hits = model.sample(cx, cy, F, R, inclusive, cap)
    for bits, h in ((0, hits[2]), (4, hits[1]), (1, hits[0])):
        got = _host(lib, [cx], [cy], F, R, inclusive, cap, bits)
        assert tuple(int(a[0]) for a in got) == (o, v, s, h), (c, F, cap, R, inclusive, bits)
    return o, v, s


@pytest.mark.parametrize("F", FS)
def test_fixed_point_and_cycle_two(lib, F):
    assert exact.limbs_for(F) in (2, 8, 24)
    # c = 0: z_2 == z_1, proved at the first step
    assert _both(lib, (0, 0), F, 1000) == (model.PROVED, 1000, 1)
    # c = -1: -1, 0, -1: z_3 == z_1 fails only because the checkpoint moved to z_2 at n = 2; z_4 == z_2
    assert _both(lib, (-1, 0), F, 1000) == (model.PROVED, 1000, 3)


@pytest.mark.parametrize("F", FS)
def test_minus_two_strict_and_inclusive(lib, F):
    # strict: z_1 = -2, then the fixed point 2 (|z|^2 == 4 never exceeds 4): z_3 == z_2, proved at n = 3 after two steps
    assert _both(lib, (-2, 0), F, 1000, R=4, inclusive=False) == (model.PROVED, 1000, 2)
    # inclusive: z_1 escapes
    assert _both(lib, (-2, 0), F, 1000, R=4, inclusive=True) == (model.ESCAPED, 0, 1)


@pytest.mark.parametrize("F", FS)
def test_parabolic_point_is_capped_and_unproved(lib, F):
    assert _both(lib, (Fraction(1, 4), 0), F, 5000) == (model.CAPPED, 5000, 5001)


def test_a_proof_behind_a_power_of_two(lib):
    """c = -0.5 + 0.5i falls into an attracting fixed point; the state stops moving once the contraction is below one unit of the
    last place, and the proof lands a few steps behind the next power of two: at n = 4101 with F 54 and at n = 16389 with F 214
    (the sample holds z_n after n - 1 steps)."""
    c = (Fraction(-1, 2), Fraction(1, 2))
    assert _both(lib, c, 54, 20000) == (model.PROVED, 20000, 4100)
    assert _both(lib, c, 214, 20000) == (model.PROVED, 20000, 16388)
    for F in (246, 758):
        o, v, s = _both(lib, c, F, 200000)
        n = s + 1
        assert o == model.PROVED and n >= 16389 and n - (1 << (n.bit_length() - 1)) < 64, (F, n)


def test_caps_around_a_proof(lib):
    """The sample is proved by its 4100th step, which leaves it holding z_4101.  With a cap of 4099 that step finds n == cap + 1
    and ends the sample unproved.  Caps of 4100 and 4101 are proved, with the cap as the value."""
    c = (Fraction(-1, 2), Fraction(1, 2))
    assert _both(lib, c, 54, 4099) == (model.CAPPED, 4099, 4100)
    assert _both(lib, c, 54, 4100) == (model.PROVED, 4100, 4100)
    assert _both(lib, c, 54, 4101) == (model.PROVED, 4101, 4100)
    assert _both(lib, c, 54, 4098) == (model.CAPPED, 4098, 4099)


def test_frame_64x48(lib):
    """bbox (-2.2, -1.2) .. (1.0, 1.2) at 64 x 48, F 54, R 4, cap 20 000: every sample's outcome, value, steps and compares; the
    frame holds all three kinds, and the check cuts the steps to less than a tenth."""
    w, h, F, cap = 64, 48, 54, 20000
    minx, miny, maxx, maxy = (Fraction(s) for s in ("-2.2", "-1.2", "1.0", "1.2"))
    fix = lambda q: (q.numerator << F) // q.denominator
    ax = [fix(minx + (maxx - minx) * x / w) for x in range(w)]
    ay = [fix(maxy - (maxy - miny) * y / h) for y in range(h)]
    m = model.frame(ax, ay, F, 4, False, cap)
    assert m.kinds() == (2462, 580, 30)
    assert (int(m.steps_off.sum()), int(m.steps.sum())) == (12218890, 1016856)
    cxs, cys = ax * h, [v for v in ay for _ in range(w)]
    for bits, col in ((0, 2), (4, 1)):
        o, v, s, cmp_ = _host(lib, cxs, cys, F, 4, False, cap, bits)
        assert np.array_equal(o, m.outcome) and np.array_equal(v, m.value) and np.array_equal(s, m.steps)
        assert np.array_equal(cmp_, m.hits[:, col])
    assert m.hit_totals[1] > 50 * int(m.proved.sum())  # the 4-bit fingerprint makes the full compare say "no"


def test_the_recorded_model_is_the_models(native_libs):
    """tests/golden/exact_cycle_model.json (what tests/test_gpu_exact_cycle.py takes for the model's word on its 64 x 48 frames):
    the frame at 54 fractional bits run again whole, the others on every 13th sample."""
    import json
    from fractalshark_amd import inputs
    with open(model.RECORD) as f:
        fx = json.load(f)
    w, h, cap = fx["width"], fx["height"], fx["cap"]
    v = inputs.View(*fx["bbox"], w, h)
    assert (w, h, cap, len(fx["frames"])) == (64, 48, 20000, 5)
    for F, R, inclusive in ((54, 4, False), (246, 4, False), (758, 4, False), (246, 256, False), (246, 4, True)):
        cx, cy = exact.axes(v, F)
        rec = model.recorded(model.record_key(w, h, F, R, inclusive, cap), model.axes_crc(cx, cy), cap)
        assert rec is not None and len(rec.steps) == w * h and min(rec.kinds()) > 0
        only = None if F == 54 else set(range(0, w * h, 13))
        live = model.frame(model.from_limbs(cx), model.from_limbs(cy), F, R, inclusive, cap, only)
        pick = np.arange(w * h) if only is None else np.array(sorted(only))
        assert np.array_equal(live.outcome[pick], rec.outcome[pick]) and np.array_equal(live.steps[pick], rec.steps[pick])
        if only is None:
            assert live.hit_totals == rec.hit_totals
