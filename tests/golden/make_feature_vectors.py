#!/usr/bin/env python3
"""The Feature Finder scan of View 5 through the CPU checker -> tests/golden/feature_vectors.json.

The reference's PTScan (FeatureFinderOrchestrator.cpp:485-559): the 12 x 12 grid of a 192 x 108 window on View 5,
HDRFloat<float>, IterType uint32_t, the period search capped at the view's iteration limit (4 718 592), every evaluation made by
tests/feature/feature_ref.cpp (the restatement of FeatureFinder::Evaluate_PT / the Direct fallback on the oracle's arithmetic).
What is stored is the scan's result: per found point its grid index, cx / cy / intrinsic radius as decimal strings, period and
residual2.  tests/test_gpu_feature_finder.py runs the same scan with every evaluation on the GPU and compares.
Usage: python tests/golden/make_feature_vectors.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from fractalshark_amd import features, inputs  # noqa: E402
from test_feature_finder_cpu import checker_evaluator  # noqa: E402

WIDTH, HEIGHT, MAX_ITERS = 192, 108, 4718592


def main():
    v = inputs.View.builtin(5, WIDTH, HEIGHT)
    ob = inputs.Orbit(v)
    found = features.scan(v, ob, checker_evaluator(ob, 4, threads=os.cpu_count() or 1), max_iters=MAX_ITERS)
    out = {"view": 5, "width": WIDTH, "height": HEIGHT, "max_iters": MAX_ITERS, "T": "HDRFloat<float>", "iter_bytes": 4,
           "found": [dict(p, residual2=list(p["residual2"])) for p in found]}
    with open(os.path.join(HERE, "feature_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%d points" % len(found))


if __name__ == "__main__":
    main()
