#!/usr/bin/env python3
"""The 86 found points of the View 5 Feature Finder fixture (tests/golden/feature_vectors.json) refined to nuclei on the GPU
(features.refine_found: the secant loop of exact.refine_points over fs_exact_eval_points), compared point by point -- status,
refined c, atom period, evaluations -- with the same loop on Python integers.  By default at the 704 fractional bits and the rounds
of the model's record (tests/golden/feature_refine_vectors.json, written by tests/golden/make_feature_refine_vectors.py), on the lane
path, against that record.  --frac-bits F, --rounds N: another precision or round count; beyond 758 bits the runs take the wide path
(fs_exact_eval_points_wide), and where the record does not hold the asked F and N the comparison is with tests/_point_model.py,
run here on the CPU (slow at many points: limit them with --points, or pass --no-compare).  Prints the time of every evaluator call
and one JSON line; exit status 1 when a point differs.
Usage: python tools/refine_features.py [--points K[,K...]] [--frac-bits F] [--rounds N] [--no-compare]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fractalshark_amd import GPURenderer, exact, features  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="", help="comma-separated fixture indices (default: all)")
    ap.add_argument("--frac-bits", type=int, default=None, help="fractional bits (default: the record's 704); beyond 758: the wide path")
    ap.add_argument("--rounds", type=int, default=None, help="secant rounds at the most (default: the record's)")
    ap.add_argument("--no-compare", action="store_true")
    args = ap.parse_args()
    with open(os.path.join(GOLDEN, "feature_vectors.json")) as f:
        found = json.load(f)["found"]
    with open(os.path.join(GOLDEN, "feature_refine_vectors.json")) as f:
        rec = json.load(f)
    F = rec["frac_bits"] if args.frac_bits is None else args.frac_bits
    rounds = rec["rounds"] if args.rounds is None else args.rounds
    recorded = (F, rounds) == (rec["frac_bits"], rec["rounds"])
    wide = F > exact.MAX_FRAC_BITS
    pick = [int(k) for k in args.points.split(",")] if args.points else list(range(len(found)))
    if GPURenderer.TestCudaIsWorking() == 0:
        raise SystemExit("no usable HIP device")
    r = GPURenderer(0)
    calls = []
    inner = exact.eval_points

    def timed(renderer, cxs, cys, lengths, frac_bits, bailout=256, inclusive=False, wide=False):
        t0 = time.perf_counter()
        out = inner(renderer, cxs, cys, lengths, frac_bits, bailout, inclusive, wide)
        dt = time.perf_counter() - t0
        st = renderer.exact_stats()
        calls.append(dt)
        print("call %2d: %3d runs, longest %6d, %9d %s steps, %3d launches, %.3f s" % (
            len(calls), len(cxs), max(lengths), st["lane_steps"], "wave" if wide else "lane", st["launches"], dt), flush=True)
        return out

    exact.eval_points = timed
    t0 = time.perf_counter()
    try:
        got = features.refine_found(r, [found[k] for k in pick], frac_bits=F, rounds=rounds, wide=wide)
    finally:
        exact.eval_points = inner
    total = time.perf_counter() - t0
    r.close()
    differ = []
    model_seconds = None
    if not args.no_compare and not recorded:
        import _point_model as model
        t0 = time.perf_counter()
        wants = [model.refine(*model.fixture_point(found[k], F), F, rounds=rounds) for k in pick]
        model_seconds = round(time.perf_counter() - t0, 3)
    for i, (k, g) in enumerate(zip(pick, got)):
        if args.no_compare:
            continue
        if recorded:
            q = rec["points"][k]
            want = (q["status"], None if q["cx"] is None else (int(q["cx"]), int(q["cy"])), q["atom"], q["evaluations"])
        else:
            want = (wants[i]["status"], wants[i]["c"], wants[i]["atom"], wants[i]["evaluations"])
        if (g["status"], g["c"], g["atom"], g["evaluations"]) != want:
            differ.append(k)
    status = lambda s: sum(1 for g in got if g["status"] == s)
    line = {"frac_bits": F, "rounds_limit": rounds, "path": "wide" if wide else "lane", "points": len(pick), "fixed": status("fixed"),
            "rounds": status("rounds"), "stalled": status("stalled"),
            "escaped": status("escaped"), "converged": sum(1 for g in got if g["converged"]),
            "atom_periods": sorted({g["atom"] for g in got if g["converged"]}),
            "calls": len(calls), "eval_seconds": round(sum(calls), 3), "total_seconds": round(total, 3),
            "compared_with": None if args.no_compare else "record" if recorded else "model", "model_seconds": model_seconds,
            "differ_from_record": differ}
    print(json.dumps(line))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
