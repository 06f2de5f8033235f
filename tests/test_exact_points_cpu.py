"""CPU-only: point runs and the secant refinement (fs_exact_eval_points, exact.points, exact.refine_points) against
tests/_point_model.py, the definitions on Python integers.  fsx::point_run of csrc/exact_atom_math.hpp -- the text the kernels
compile -- is built for the host with g++ (tests/exact/exact_points_host.cpp); exact.refine_points runs on the model's evaluator.
Every comparison is an equality of integers."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _point_model as model
from fractalshark_amd import exact

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "exact", "exact_points_host.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "fractalshark_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("exact_atom_math.hpp", "exact_cycle_math.hpp", "exact_math.hpp")]
SO = os.path.join(HERE, "exact", "libexact_points_host.so")

FS = (54, 246, 758)  # frac_bits of 2, 8 and 24 limbs, the largest each holds
LENGTHS = (1, 2, 3, 64, 65, 1000)
KEYS = ("status", "c", "atom", "evaluations", "converged")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or max(os.path.getmtime(p) for p in [SRC] + HDRS) > os.path.getmtime(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC], check=True)
    h = C.CDLL(SO)
    h.exp_point_runs.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32,
                                 C.c_void_p, C.c_void_p]
    return h


def _host(lib, cxs, cys, lengths, F, R, inclusive, key_bits=0):
    """The header's loop on the runs: [(v, A, endpoint or None, the endpoint's limbs all zero)]."""
    L, n = exact.limbs_for(F), len(cxs)
    cx = np.ascontiguousarray(exact._to_limbs(cxs, L).T)
    cy = np.ascontiguousarray(exact._to_limbs(cys, L).T)
    ln = np.array(lengths, np.uint64)
    out, end = np.zeros((n, 3), np.uint64), np.full((n, 2 * L), 0xDEADBEEF, np.uint32)
    assert lib.exp_point_runs(L, n, cx.ctypes.data, cy.ctypes.data, ln.ctypes.data, F, R, 1 if inclusive else 0, key_bits, out.ctypes.data,
                              end.ctypes.data) == 0
    xs, ys = exact._from_limbs(end[:, :L].T), exact._from_limbs(end[:, L:].T)
    return [(int(out[i, 0]), int(out[i, 1]), (xs[i], ys[i]) if int(out[i, 0]) == lengths[i] else None, not end[i].any()) for i in range(n)]


def _fix(c, F):
    return tuple(model.fix(Fraction(v), F) for v in c)


POINTS = [(0, 0), (-1, 0), (Fraction(1, 4), 0), (Fraction(5, 2), Fraction(1, 3)), (-2, 0), (Fraction(-3, 4), Fraction(1, 20)),
          (Fraction(-12253, 100000), Fraction(74484, 100000)), (Fraction(35, 2), Fraction(1, 3))]


@pytest.mark.parametrize("F,R", [(54, 4), (246, 4), (758, 4), (246, 256)])
@pytest.mark.parametrize("inclusive", [False, True])
def test_point_run_equals_the_model(lib, F, R, inclusive):
    """Lengths 1, 2, 3, 64, 65, 1000 and, for the c that escapes after a few dozen steps, lengths below, at and above E; c = 0, -1,
    1/4, |c| > 2 and |c| > 16 (v = 0, A = 0, no endpoint: under R = 4, under both), -2 (escapes at once when inclusive under R = 4),
    a c next to the period-3 nucleus."""
    esc = _fix(POINTS[5], F)
    E = model.run(esc[0], esc[1], F, R, inclusive, 10 ** 6)[0] + 1
    assert 10 < E < 1000
    cxs, cys, lengths = [], [], []
    for c in POINTS:
        a, b = _fix(c, F)
        for p in LENGTHS + ((E - 2, E - 1, E, E + 1) if c is POINTS[5] else ()):
            cxs.append(a), cys.append(b), lengths.append(p)
    want = [model.run(a, b, F, R, inclusive, p) for a, b, p in zip(cxs, cys, lengths)]
    for bits in (0, 6):  # the full key and the narrowest: the same values
        got = _host(lib, cxs, cys, lengths, F, R, inclusive, bits)
        for g, w, c, p in zip(got, want, zip(cxs, cys), lengths):
            assert g[:3] == w, (F, R, inclusive, bits, c, p, g, w)
            assert g[3] == (w[2] is None or w[2] == (0, 0))  # short of its length: every limb zero
    # what the definitions say about the simple points
    run = lambda c, p: model.run(*_fix(c, F), F, R, inclusive, p)
    assert run((0, 0), 1000) == (1000, 1, (0, 0)) and run((-1, 0), 1000)[:2] == (1000, 2)
    assert run((-1, 0), 3) == (3, 2, (-1 << F, 0)) and run((-1, 0), 2) == (2, 2, (0, 0)) and run((-1, 0), 1) == (1, 1, (-1 << F, 0))
    assert run(POINTS[7], 1000) == (0, 0, None) and (R != 4 or run(POINTS[3], 1000) == (0, 0, None))  # c itself escapes
    assert run((Fraction(1, 4), 0), 1000)[:2] == (1000, 1)
    assert run((-2, 0), 64)[:2] == ((0, 0) if inclusive and R == 4 else (64, 1))
    assert run(POINTS[5], E - 1)[0] == E - 1 and run(POINTS[5], E - 1)[2] is not None  # escapes after the length
    assert run(POINTS[5], E) == (E - 1, run(POINTS[5], E - 1)[1], None)  # at it
    assert run(POINTS[5], E + 1)[2] is None  # before it
    assert run(POINTS[6], 1000)[:2] == (1000, 3)


def test_points_are_floors_of_exact_rationals():
    vals = ["-1.5", "0.1", "-0.1", "3e-5", "-5.4820574807047570845821256754673302937669927823522733666984672177847259238050304e-1",
            Fraction(1, 3), Fraction(-1, 3), 0, "31.999"]
    for F in (0, 54, 246, 704, 758):
        ints, arr = exact.points(vals, F)
        L = exact.limbs_for(F)
        assert arr.dtype == np.uint32 and arr.shape == (L, len(vals))
        for v, i, col in zip(vals, ints, arr.T):
            q = Fraction(v) * (1 << F)
            assert i <= q < i + 1
            assert [int(w) for w in col] == [((i % (1 << (32 * L))) >> (32 * l)) & 0xFFFFFFFF for l in range(L)]
        assert exact._from_limbs(arr) == ints
    assert exact.points(["0.5"], 54, limbs=4)[1].shape == (4, 1)
    with pytest.raises(ValueError):
        exact.points(["1e30"], 54)


def _same(got, want, what):
    assert {k: got[k] for k in KEYS} == {k: want[k] for k in KEYS}, (what, got, want)
    assert got["log2"] == want["log2"]


@pytest.mark.parametrize("F", [54, 246])
@pytest.mark.parametrize("offset", ["1e-3", "1e-5"])
def test_refine_small_nuclei(F, offset):
    """Periods 1 .. 5 from next to their nuclei: exact.refine_points on the model's evaluator equals the model's own loop, all in one
    batch, and every point ends with A = p."""
    o = model.fix(offset, F)
    c0s = [(model.fix(x, F) + o, model.fix(y, F) + o // 2) for _, x, y in model.SMALL_NUCLEI]
    deltas = [model.delta_of(offset, F)] * len(c0s)
    periods = [p for p, _, _ in model.SMALL_NUCLEI]
    calls = []

    def evaluate(cxs, cys, lengths):
        calls.append(len(cxs))
        return model.evaluator(F)(cxs, cys, lengths)

    got = exact.refine_points(evaluate, c0s, deltas, periods, F)
    assert calls[0] == 2 * len(c0s) and all(a >= b for a, b in zip(calls[1:], calls[2:])) and len(calls) <= 17
    for k, g in enumerate(got):
        _same(g, model.refine(c0s[k], deltas[k], periods[k], F), (F, offset, periods[k]))
        assert g["converged"] and g["atom"] == periods[k] and g["status"] == "fixed", (F, offset, g)
    # `rounds` counts passes of the update loop
    short = exact.refine_points(model.evaluator(F), c0s, deltas, periods, F, rounds=2)
    for k, g in enumerate(short):
        _same(g, model.refine(c0s[k], deltas[k], periods[k], F, rounds=2), (F, offset, periods[k], "rounds=2"))
        assert g["evaluations"] <= 4
    assert any(g["status"] == "rounds" for g in short)
    assert exact.refine_points(model.evaluator(F), [], [], [], F) == []


def test_refine_fixture_points_equal_the_model_and_the_record():
    """Points 0, 10, 42 and 43 of the View 5 fixture at F = 704 converge to A = their period; 44 escapes inside the loop, 9 at the
    start.  One batch through exact.refine_points, against the model's loop point by point and against the record
    (tests/golden/feature_refine_vectors.json, which tests/golden/make_feature_refine_vectors.py writes with the same model)."""
    rec = model.record()
    F = rec["frac_bits"]
    found = model.fixture()
    assert (F, rec["rounds"], rec["bailout"], len(rec["points"]), len(found)) == (704, 16, 256, 86, 86)
    count = lambda s: sum(1 for q in rec["points"] if q["status"] == s)
    assert (count("fixed"), count("rounds"), count("escaped"), count("stalled")) == (74, 1, 11, 0)
    assert sum(1 for q in rec["points"] if q["converged"]) == 75
    pick = [0, 10, 42, 43, 44, 9]
    starts = [model.fixture_point(found[k], F) for k in pick]
    got = exact.refine_points(model.evaluator(F), [s[0] for s in starts], [s[1] for s in starts], [s[2] for s in starts], F, rec["rounds"])
    for k, g, (c0, delta, p) in zip(pick, got, starts):
        _same(g, model.refine(c0, delta, p, F, rec["rounds"]), k)
        q = rec["points"][k]
        want_c = None if q["cx"] is None else (int(q["cx"]), int(q["cy"]))
        assert (g["status"], g["c"], g["atom"], g["evaluations"], g["converged"]) == (q["status"], want_c, q["atom"], q["evaluations"],
                                                                                    q["converged"]), k
    for g, (_, _, p) in list(zip(got, starts))[:4]:
        assert g["converged"] and g["atom"] == p and g["status"] in ("fixed", "rounds")
    assert got[4]["status"] == "escaped" and got[4]["evaluations"] > 2
    assert got[5]["status"] == "escaped" and got[5]["evaluations"] == 2 and got[5]["c"] is None and not got[5]["converged"]
