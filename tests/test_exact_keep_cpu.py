"""CPU-only: the park-and-resume rule of csrc/exact_cycle_math.hpp (fs_set_exact_keep, fs_render_exact_continue) -- a sample run to
a cap N1, parked, and resumed to N2 -- built for the host with g++ as a program of its own (tests/exact/exact_keep_host.cpp) against
the rule restated on Python integers (tests/_cycle_model.py) run to N1 and straight to N2: the first run is the model's at N1 (a
sample that meets the cap is capped and UNPROVED there), the two runs together end as the model does at N2, and their steps and
checkpoint read-backs add up to the model's exactly -- the cycle check at n = N1 + 2 is neither skipped nor run twice."""
import os
import subprocess
from fractions import Fraction

import pytest

import _cycle_model as model
from fractalshark_amd import exact

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "exact", "exact_keep_host.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "fractalshark_amd", "csrc")
HDRS = [os.path.join(CSRC, "exact_cycle_math.hpp"), os.path.join(CSRC, "exact_math.hpp")]
EXE = os.path.join(HERE, "exact", "build", "exact_keep_host")

F = 54
HALF = (Fraction(-1, 2), Fraction(1, 2))  # falls into an attracting fixed point; proved a few steps behind 4096
POINTS = [((0, 0), False), ((-1, 0), False), ((-2, 0), False), ((-2, 0), True), ((Fraction(1, 4), 0), False), (HALF, False)]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or max(os.path.getmtime(p) for p in [SRC] + HDRS) > os.path.getmtime(EXE):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", EXE, SRC], check=True)
    return EXE


def _fix(v, frac_bits=F):
    v = Fraction(v)
    return (v.numerator << frac_bits) // v.denominator


def _host(exe, cxs, cys, R, inclusive, n1, n2, check=True, fp_bits=0, frac_bits=F):
    """The program on the samples (Python integers): a list of (run1, run2, n_parked), a run = (outcome, value, steps, compares)."""
    L = exact.limbs_for(frac_bits)
    words = lambda v: " ".join("%x" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(L))
    text = "%d %d %d %d %d %d %d %d %d\n" % (L, frac_bits, R, 1 if inclusive else 0, n1, n2, fp_bits, 1 if check else 0, len(cxs))
    text += "".join("%s %s\n" % (words(a), words(b)) for a, b in zip(cxs, cys))
    p = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True)
    rows = [[int(t) for t in line.split()] for line in p.stdout.splitlines()]
    assert len(rows) == len(cxs) and all(len(r) == 9 for r in rows)
    return [(tuple(r[0:4]), tuple(r[4:8]), r[8]) for r in rows]


def _expect(cx, cy, R, inclusive, n1, n2, col=2):
    """What the model says the two runs must be.  col: the fingerprint column of the model's hits (2: all 64 bits)."""
    o1, v1, s1, h1 = model.sample(cx, cy, F, R, inclusive, n1)
    run1 = (o1, v1, s1, h1[col])
    if o1 != model.CAPPED or n2 <= n1:
        return run1, (model.CAPPED, n2, 0, 0), 0
    o2, v2, s2, h2 = model.sample(cx, cy, F, R, inclusive, n2)
    return run1, (o2, v2, s2 - s1, h2[col] - h1[col]), n1 + 1


def _proof_n():
    """The n at which the model proves -0.5 + 0.5i at F = 54: it holds z_n after n - 1 steps."""
    o, _, s, _ = model.sample(_fix(HALF[0]), _fix(HALF[1]), F, 4, False, 1 << 20)
    assert o == model.PROVED
    return s + 1


def test_resume_boundaries(exe):
    """Every point with N1 such that the resume boundary n = N1 + 2 is a power of two (the checkpoint is retaken by the resumed
    sample), is the n of -0.5 + 0.5i's proof (the deferred check IS the proof), and lies one below and one above it."""
    n_p = _proof_n()
    assert n_p - (1 << (n_p.bit_length() - 1)) < 64 and n_p > 4096  # a few steps behind a power of two (4101)
    n1s = [0, 1, 2, 6, 1022, 4094, n_p - 2, n_p - 3, n_p - 1]
    n2 = 6000
    seen_deferred_proof = False
    for (c, inclusive) in POINTS:
        cx, cy = _fix(c[0]), _fix(c[1])
        for n1 in n1s:
            for bits, col in ((0, 2), (4, 1), (1, 0)):
                got = _host(exe, [cx], [cy], 4, inclusive, n1, n2, fp_bits=bits)[0]
                assert got == _expect(cx, cy, 4, inclusive, n1, n2, col), (c, inclusive, n1, bits, got)
            if got[0][0] == model.CAPPED and got[1] == (model.PROVED, n2, 0, 1):
                seen_deferred_proof = True
    assert seen_deferred_proof  # (a resumed sample proved by its deferred check alone, with no step of its own)
    # the proof's own boundary, spelled out: capped and unproved at N1 = n_p - 2, proved by the deferred check on resume
    cx, cy = _fix(HALF[0]), _fix(HALF[1])
    r1, r2, parked = _host(exe, [cx], [cy], 4, False, n_p - 2, n2)[0]
    assert r1[:3] == (model.CAPPED, n_p - 2, n_p - 1) and r2[:3] == (model.PROVED, n2, 0) and parked == n_p - 1


def test_chain_and_equal_caps(exe):
    """N2 == N1 resumes nothing; the parabolic point stays capped and unproved however the cap is cut."""
    cx, cy = _fix(Fraction(1, 4)), 0
    r1, r2, parked = _host(exe, [cx], [cy], 4, False, 100, 100)[0]
    assert (r1[:3], r2, parked) == ((model.CAPPED, 100, 101), (model.CAPPED, 100, 0, 0), 0)
    r1, r2, parked = _host(exe, [cx], [cy], 4, False, 1022, 5000)[0]
    assert (r1[:3], r2[:3], parked) == ((model.CAPPED, 1022, 1023), (model.CAPPED, 5000, 5001 - 1023), 1023)


def test_without_the_check(exe):
    """check off (the C = false kernels): no proof and no read-back; the two runs' steps add up to those of one run."""
    for (c, inclusive) in POINTS:
        cx, cy = _fix(c[0]), _fix(c[1])
        o, v, s, _ = model.sample(cx, cy, F, 4, inclusive, 3000)
        steps_off = s if o == model.ESCAPED else 3001
        for n1 in (0, 2, 1022):
            r1, r2, _ = _host(exe, [cx], [cy], 4, inclusive, n1, 3000, check=False)[0]
            if o == model.ESCAPED and v < n1 + 1:
                assert r1 == (model.ESCAPED, v, s, 0) and r2[2] == 0
            else:
                assert r1 == (model.CAPPED, n1, n1 + 1, 0)
                assert r2 == ((model.ESCAPED, v, steps_off - n1 - 1, 0) if o == model.ESCAPED else
                              (model.CAPPED, 3000, steps_off - n1 - 1, 0))


def test_frame_64x48(exe):
    """bbox (-2.2, -1.2) .. (1.0, 1.2) at 64 x 48, F 54, R 4: every sample to N1 = 100, parked, resumed to 20 000 -- the cap of
    tests/test_exact_cycle_cpu.py's frame -- against the model at both caps."""
    w, h, n1, n2 = 64, 48, 100, 20000
    minx, miny, maxx, maxy = (Fraction(s) for s in ("-2.2", "-1.2", "1.0", "1.2"))
    ax = [_fix(minx + (maxx - minx) * x / w) for x in range(w)]
    ay = [_fix(maxy - (maxy - miny) * y / h) for y in range(h)]
    cxs, cys = ax * h, [v for v in ay for _ in range(w)]
    m1, m2 = model.frame(ax, ay, F, 4, False, n1), model.frame(ax, ay, F, 4, False, n2)
    assert m2.kinds() == (2462, 580, 30)
    got = _host(exe, cxs, cys, 4, False, n1, n2)
    kept = 0
    for i, (r1, r2, parked) in enumerate(got):
        assert r1 == (int(m1.outcome[i]), int(m1.value[i]), int(m1.steps[i]), int(m1.hits[i, 2])), i
        if m1.outcome[i] == model.CAPPED:
            kept += 1
            assert parked == n1 + 1
            assert r2 == (int(m2.outcome[i]), int(m2.value[i]), int(m2.steps[i] - m1.steps[i]), int(m2.hits[i, 2] - m1.hits[i, 2])), i
        else:
            assert r2 == (model.CAPPED, n2, 0, 0) and parked == 0
            assert (m1.outcome[i], m1.steps[i]) == (m2.outcome[i], m2.steps[i])
    assert kept == int((m1.outcome == model.CAPPED).sum()) and 0 < kept < w * h
    # the work of the two runs together is the work of one
    assert sum(r1[2] + r2[2] for r1, r2, _ in got) == int(m2.steps.sum())
