#!/usr/bin/env python3
"""The 86 found points of the View 5 Feature Finder fixture (tests/golden/feature_vectors.json) refined to nuclei on the GPU at 704
fractional bits (features.refine_found: the secant loop of exact.refine_points over fs_exact_eval_points), compared point by point
-- status, refined c, atom period, evaluations -- with the model's record (tests/golden/feature_refine_vectors.json, written by
tests/golden/make_feature_refine_vectors.py on Python integers).  Prints the time of every fs_exact_eval_points call and one JSON
line; exit status 1 when a point differs from the record.
Usage: python tools/refine_features.py [--points K[,K...]] [--no-compare]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fractalshark_amd import GPURenderer, exact, features  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="", help="comma-separated fixture indices (default: all)")
    ap.add_argument("--no-compare", action="store_true")
    args = ap.parse_args()
    with open(os.path.join(GOLDEN, "feature_vectors.json")) as f:
        found = json.load(f)["found"]
    with open(os.path.join(GOLDEN, "feature_refine_vectors.json")) as f:
        rec = json.load(f)
    F, rounds = rec["frac_bits"], rec["rounds"]
    pick = [int(k) for k in args.points.split(",")] if args.points else list(range(len(found)))
    if GPURenderer.TestCudaIsWorking() == 0:
        raise SystemExit("no usable HIP device")
    r = GPURenderer(0)
    calls = []
    inner = exact.eval_points

    def timed(renderer, cxs, cys, lengths, frac_bits, bailout=256, inclusive=False):
        t0 = time.perf_counter()
        out = inner(renderer, cxs, cys, lengths, frac_bits, bailout, inclusive)
        dt = time.perf_counter() - t0
        st = renderer.exact_stats()
        calls.append(dt)
        print("call %2d: %3d runs, longest %6d, %9d lane steps, %3d launches, %.3f s" % (len(calls), len(cxs), max(lengths),
                                                                                        st["lane_steps"], st["launches"], dt), flush=True)
        return out

    exact.eval_points = timed
    t0 = time.perf_counter()
    try:
        got = features.refine_found(r, [found[k] for k in pick], frac_bits=F, rounds=rounds)
    finally:
        exact.eval_points = inner
    total = time.perf_counter() - t0
    r.close()
    differ = []
    for k, g in zip(pick, got):
        q = rec["points"][k]
        want = (q["status"], None if q["cx"] is None else (int(q["cx"]), int(q["cy"])), q["atom"], q["evaluations"])
        if not args.no_compare and (g["status"], g["c"], g["atom"], g["evaluations"]) != want:
            differ.append(k)
    status = lambda s: sum(1 for g in got if g["status"] == s)
    line = {"frac_bits": F, "points": len(pick), "fixed": status("fixed"), "rounds": status("rounds"), "stalled": status("stalled"),
            "escaped": status("escaped"), "converged": sum(1 for g in got if g["converged"]),
            "atom_periods": sorted({g["atom"] for g in got if g["converged"]}),
            "calls": len(calls), "eval_seconds": round(sum(calls), 3), "total_seconds": round(total, 3),
            "differ_from_record": differ}
    print(json.dumps(line))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
