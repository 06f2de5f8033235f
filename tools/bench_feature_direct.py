#!/usr/bin/env python3
"""Times of the Feature Finder's Direct evaluator (fs_feature_eval_direct) for DESIGN.md section 6.1, against the CPU checker
(tests/feature/feature_direct_ref.cpp): one wave's step, the View 0 12 x 12 DirectScan, and period maps of View 0.
Prints one JSON line.  Usage: python tools/bench_feature_direct.py [--maps 256,1024,2048] [--cap 8192]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fractalshark_amd import GPURenderer, T_HDR32, T_HDR64, features, inputs  # noqa: E402
from test_feature_direct_cpu import direct_checker_evaluator, direct_checker_lib  # noqa: E402


def timed(f, repeats=3):
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def wave_step_ns(r, T):
    """64 lanes in lockstep at the period-3 nucleus, fixed periods 2^16 and 2^20: the difference, per step."""
    din, dout, dreal = features.records(T == T_HDR64)
    rin, rout, rad = np.zeros(64, din), np.zeros(64, dout), np.zeros(1, dreal)
    rin["c"]["re"], rin["c"]["im"] = -0.12256116687665362, 0.7448617666197442
    ts = []
    for p in (1 << 16, 1 << 20):
        rin["period"] = p
        t, _ = timed(lambda: r.FeatureEvalDirect(T, 4, features.FIXED, rad, p, rin, rout))
        assert (rout["status"] == features.OK_DIRECT).all()
        ts.append(t)
    return (ts[1] - ts[0]) / ((1 << 20) - (1 << 16)) * 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="256,1024,2048")
    ap.add_argument("--cap", type=int, default=8192)
    a = ap.parse_args()
    r = GPURenderer(0)
    res = {"cap": a.cap}
    r.FeatureEvalDirect(T_HDR32, 4, features.FIND, np.zeros(1, features.REAL_HDR32), 1, np.zeros(1, features.FEATURE_IN_HDR32),
                        np.zeros(1, features.FEATURE_OUT_HDR32))  # (first launch: code load)
    for T, name in ((T_HDR32, "hdr32"), (T_HDR64, "hdr64")):
        is64 = T == T_HDR64
        res["wave_step_ns_" + name] = round(wave_step_ns(r, T), 1)
        v = inputs.View.builtin(0, 192, 108)
        t_gpu, found = timed(lambda: features.find_periodic_points_direct(r, v, T=T, max_iters=a.cap))
        t_c1, f1 = timed(lambda: features.scan_direct(v, is64, direct_checker_evaluator(is64, 4, 1), max_iters=a.cap))
        t_c16, f16 = timed(lambda: features.scan_direct(v, is64, direct_checker_evaluator(is64, 4, 16), max_iters=a.cap))
        assert found == f1 == f16
        rin, rad = features.direct_grid(v, is64, 12, 12)
        rout = np.zeros(len(rin), features.records(is64)[1])
        t_find, _ = timed(lambda: r.FeatureEvalDirect(T, 4, features.FIND, rad, a.cap, rin, rout))
        res["scan12_" + name] = {"found": len(found), "gpu_ms": round(t_gpu * 1e3, 2), "gpu_find_round_ms": round(t_find * 1e3, 3),
                                 "checker_1t_ms": round(t_c1 * 1e3, 2), "checker_16t_ms": round(t_c16 * 1e3, 2)}
    lib = direct_checker_lib()
    for n in [int(x) for x in a.maps.split(",") if x]:
        v = inputs.View.builtin(0, n, n)
        for T, name in ((T_HDR32, "hdr32"), (T_HDR64, "hdr64")):
            is64 = T == T_HDR64
            t_map, m = timed(lambda: features.period_map(r, v, n, n, T=T, max_iters=a.cap), 2)
            t_grid, (rin, rad) = timed(lambda: features.direct_grid(v, is64, n, n), 1)
            rout = np.zeros(len(rin), features.records(is64)[1])
            t_eval, _ = timed(lambda: r.FeatureEvalDirect(T, 4, features.FIND, rad, a.cap, rin, rout), 2)
            ref, steps = np.zeros_like(rout), np.zeros(len(rin), np.uint64)
            t_chk, _ = timed(lambda: lib.ffr_feature_eval_direct(1 if is64 else 0, 4, 0, rad.ctypes.data, a.cap, rin.ctypes.data,
                                                                 ref.ctypes.data, len(rin), 16), 1)
            assert ref.tobytes() == rout.tobytes()
            lib.ffr_feature_eval_direct_steps(1 if is64 else 0, 4, 0, rad.ctypes.data, a.cap, rin.ctypes.data, ref.ctypes.data,
                                              len(rin), 16, steps.ctypes.data)
            w = steps.reshape(-1, 64)
            slots = float(w.max(axis=1).sum()) * 64.0
            res["map%d_%s" % (n, name)] = {
                "periods": int((m != 0).sum()), "period_map_s": round(t_map, 4), "grid_records_s": round(t_grid, 4),
                "gpu_eval_s": round(t_eval, 4), "checker_16t_s": round(t_chk, 4), "lane_steps": int(steps.sum()),
                "idle_share": round(1.0 - float(steps.sum()) / slots, 4), "longest_wave_steps": int(w.max())}
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
