#!/usr/bin/env python3
"""The Feature Finder's DirectScan of View 0 through the CPU checker -> tests/golden/feature_direct_vectors.json.

The reference's DirectScan (FeatureFinderOrchestrator.cpp:485-499, 535-551): the 12 x 12 grid of a 192 x 108 window on View 0,
HDRFloat<double>, IterType uint32_t, the period search capped at 8 192 steps, every evaluation made by
tests/feature/feature_direct_ref.cpp (the restatement of Evaluate_FindPeriod_Direct / Evaluate_PeriodResidualAndDzdc_Direct on the
oracle's arithmetic).  Stored: per found point its grid index, cx / cy / intrinsic radius as decimal strings, period and
residual2; and the period each of the 144 grid points triggers at in the search round (0: rejected).
tests/test_feature_direct_cpu.py repeats the scan; tests/test_gpu_feature_direct.py runs it with every evaluation on the GPU.
Usage: python tests/golden/make_feature_direct_vectors.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from fractalshark_amd import features, inputs  # noqa: E402
from test_feature_direct_cpu import direct_checker_evaluator, direct_first_batch  # noqa: E402

VIEW, WIDTH, HEIGHT, MAX_ITERS = 0, 192, 108, 8192


def main():
    v = inputs.View.builtin(VIEW, WIDTH, HEIGHT)
    evaluate = direct_checker_evaluator(True, 4)
    found = features.scan_direct(v, True, evaluate, max_iters=MAX_ITERS)
    mode, radius, rin = direct_first_batch(v, True, 4, MAX_ITERS)
    rout = np.zeros(len(rin), features.FEATURE_OUT_HDR64)
    evaluate(mode, radius, MAX_ITERS, rin, rout)
    periods = np.where(rout["status"] == features.OK_DIRECT, rout["period"], 0)
    out = {"view": VIEW, "width": WIDTH, "height": HEIGHT, "max_iters": MAX_ITERS, "T": "HDRFloat<double>", "iter_bytes": 4,
           "found": [dict(p, residual2=list(p["residual2"])) for p in found], "find_periods": periods.tolist()}
    with open(os.path.join(HERE, "feature_direct_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%d points found, %d of %d periods in the search round" % (len(found), int((periods != 0).sum()), len(periods)))


if __name__ == "__main__":
    main()
