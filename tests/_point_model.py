"""Point runs and the secant refinement of found points, restated on Python integers -- the model the CPU and GPU tests of
fs_exact_eval_points, exact.refine_points and features.refine_found compare with.  Written from the definitions, not from the
product's code (csrc/exact_atom_math.hpp, fractalshark_amd/exact.py).

  A run: c = (cx + i cy) / 2^F and a length p >= 1.  z_1 = c, z_{n+1} = (floor((x^2 - y^2) / 2^F) + cx, floor(2 x y / 2^F) + cy).
  N_n = x_n^2 + y_n^2, untruncated.  E is the first n at which z_n escapes (N_n > R 2^2F, >= when inclusive).  v = min(E - 1, p).
  A is the n in 1 .. v with the smallest N_n, the earliest such n; 0 when v = 0.  The endpoint is (x_p, y_p) when v == p, else none
  (the device: all limbs zero).

  The refinement of one point, period p, from c0 with the offset delta (every `//` and `>>` floors; the complex products are written
  out on integers):
      c0 given; c1 = c0 + (delta, 0)
      evaluate both; if either has v < p: status "escaped", no result
      f0, f1 = their endpoints
      repeat at most `rounds` times:
          d = f1 - f0;            if d == 0: status "stalled", stop
          q = floor(f1 conj(d) 2^F / |d|^2)  (per component)
          s = (q (c1 - c0)) >> F             (per component)
          c2 = c1 - s;            if c2 == c1: status "fixed", stop
          evaluate c2;            if v < p: status "escaped", stop
          (c0, f0, c1, f1) = (c1, f1, c2, f2)
      otherwise: status "rounds"
  The result is the evaluated iterate with the smallest N_p, the earliest on ties, with that iterate's A; converged: A == p there.
"""
import json
import math
import os

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_refine_vectors.json")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_vectors.json")


def run(cx, cy, F, R, inclusive, p):
    """(v, A, endpoint) of one run; the endpoint is (x_p, y_p) or None."""
    bail = R << (2 * F)
    x, y, n = cx, cy, 1
    A, best = 0, None
    while True:
        xx, yy = x * x, y * y
        N = xx + yy
        if N > bail or (inclusive and N == bail):
            return n - 1, A, None
        if best is None or N < best:
            A, best = n, N
        if n == p:
            return p, A, (x, y)
        x, y = ((xx - yy) >> F) + cx, ((2 * x * y) >> F) + cy
        n += 1


def evaluator(F, R=256, inclusive=False):
    """The evaluator exact.refine_points takes, made of run(): evaluate(cxs, cys, lengths) -> (values, atoms, ends)."""

    def evaluate(cxs, cys, lengths):
        res = [run(a, b, F, R, inclusive, p) for a, b, p in zip(cxs, cys, lengths)]
        return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]

    return evaluate


def log2_abs(end, F):
    """log2 |z| of an endpoint (value * 2^F as integers); -inf at zero.  A diagnostic, not part of any equality."""
    N = end[0] * end[0] + end[1] * end[1]
    return 0.5 * math.log2(N) - F if N else -math.inf


def refine(c0, delta, p, F, rounds=16, R=256, inclusive=False):
    """One point through the loop above: {status, c, atom, evaluations, converged, log2}; c = (cx, cy) as integers, None when no
    iterate was evaluated to its end."""
    evals = []  # (c, A, endpoint) of every evaluated iterate whose run reached p

    def ev(c):
        v, A, end = run(c[0], c[1], F, R, inclusive, p)
        if v == p:
            evals.append((c, A, end))
        return end

    n_eval = 2
    c1 = (c0[0] + delta, c0[1])
    f0, f1 = ev(c0), ev(c1)
    status = "rounds"
    if f0 is None or f1 is None:
        return {"status": "escaped", "c": None, "atom": None, "evaluations": n_eval, "converged": False,
                "log2": [log2_abs(e[2], F) for e in evals]}
    for _ in range(rounds):
        dx, dy = f1[0] - f0[0], f1[1] - f0[1]
        if dx == 0 and dy == 0:
            status = "stalled"
            break
        dd = dx * dx + dy * dy
        qx = ((f1[0] * dx + f1[1] * dy) << F) // dd
        qy = ((f1[1] * dx - f1[0] * dy) << F) // dd
        ex, ey = c1[0] - c0[0], c1[1] - c0[1]
        sx, sy = (qx * ex - qy * ey) >> F, (qx * ey + qy * ex) >> F
        c2 = (c1[0] - sx, c1[1] - sy)
        if c2 == c1:
            status = "fixed"
            break
        n_eval += 1
        f2 = ev(c2)
        if f2 is None:
            status = "escaped"
            break
        c0, f0, c1, f1 = c1, f1, c2, f2
    best = min(range(len(evals)), key=lambda k: (evals[k][2][0] ** 2 + evals[k][2][1] ** 2, k))
    c, A, _ = evals[best]
    return {"status": status, "c": c, "atom": A, "evaluations": n_eval, "converged": A == p,
            "log2": [log2_abs(e[2], F) for e in evals]}


def fix(value, F):
    """floor(value 2^F) of a decimal string or a Fraction."""
    from fractions import Fraction
    q = Fraction(value)
    return (q.numerator << F) // q.denominator


def delta_of(radius, F):
    """The starting offset features.refine_found takes from a found point's intrinsic radius."""
    return max(1, fix(radius, F) >> 30)


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)["found"]


def fixture_point(pt, F):
    """(c0, delta, period) of one found point of the fixture."""
    return (fix(pt["cx"], F), fix(pt["cy"], F)), delta_of(pt["intrinsic_radius"], F), int(pt["period"])


# The nuclei of periods 1 .. 5 the small tests start next to (decimal strings to a few digits: the refinement does the rest).
SMALL_NUCLEI = [(1, "0", "0"), (2, "-1", "0"), (3, "-0.1225611668766536", "0.7448617666197442"),
                (4, "-0.1565201668337551", "1.0322471089228318"), (5, "-1.6254137251233037", "0")]


def record():
    with open(RECORD) as f:
        return json.load(f)
