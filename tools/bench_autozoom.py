#!/usr/bin/env python3
"""fs_autozoom_pick against what a caller had to do without it: read the iteration buffer back (fs_render_current into
page-locked host memory) and scan it on one CPU thread (the sequential checker, tests/autozoom/autozoom_ref.cpp, the same scans
as AutoZoomer::Run).  Per heuristic, at BASELINE config C3's frame (3840x2160, uint32) and at C4's (3840x2160 x AA4 =
15360x8640, the largest frame the tests use).  The frame is View 0 rendered by the direct double kernel.

Times are host clocks around calls that end in a synchronisation of the compute stream; every shape is warmed up first; the
median and the extremes of --repeats runs are reported.  One JSON line per geometry.

  python tools/bench_autozoom.py [--repeats 20] [--skip-c4]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fractalshark_amd import GPURenderer, T_F64, _capi, autozoom, inputs  # noqa: E402
import _autozoom  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--cpu-repeats", type=int, default=3)
ap.add_argument("--skip-c4", action="store_true")
args = ap.parse_args()


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def geometry(r, name, width, height, aa):
    v = inputs.View.builtin(0, width, height, antialiasing=aa)
    W, H, n = width * aa, height * aa, v.num_iterations
    assert r.InitializeMemory(W, H, aa, None, 0, 0, 0, False) == 0
    dx, dy, minx, maxy = v.coords_direct_f64(aa)
    assert r.Render(None, minx, maxy, dx, dy, n, T=T_F64) == 0
    assert r.SyncComputeStream() == 0
    host = r.new_iter_buffer()
    assert r._lib.fs_host_register(host.ctypes.data, host.nbytes) == 0

    def read_back():
        assert r.RenderCurrent(n, host) == 0
        assert r.SyncComputeStream() == 0

    out = {"geometry": "%s: %dx%d x AA%d = %dx%d uint32, %.1f MB" % (name, width, height, aa, W, H, host.nbytes / 1e6),
           "n_iterations": n, "read_back_pinned": timed(read_back, args.repeats, 3)}
    out["read_back_pinned"]["GB_s"] = round(host.nbytes / out["read_back_pinned"]["median_ms"] / 1e6, 1)
    for hname, heur in sorted(_autozoom.HEURISTICS.items()):
        res = []

        def pick():
            err, rec = r.AutozoomPick(heur, n)
            assert err == 0
            res[:] = [rec]

        t_pick = timed(pick, args.repeats, 3)
        t_scan = timed(lambda: _autozoom.ref_pick(host, W, H, heur, n, aa), args.cpu_repeats, 1)
        ref = _autozoom.ref_pick(host, W, H, heur, n, aa)
        same = _autozoom.as_dict(res[0]) == _autozoom.as_dict(ref) if heur != autozoom.DEFAULT else \
            all(getattr(res[0], k) == getattr(ref, k) for k in _autozoom.INT_FIELDS)
        out[hname] = {"fs_autozoom_pick": t_pick, "checker_scan_one_thread": t_scan,
                      "read_back_plus_scan_median_ms": round(out["read_back_pinned"]["median_ms"] + t_scan["median_ms"], 4),
                      "pick_effective_GB_s": round(W * H * 4 / t_pick["median_ms"] / 1e6, 1),
                      "status": int(res[0].status), "target": [res[0].target_x, res[0].target_y],
                      "rescored": int(res[0].rescored), "accepted": int(res[0].accepted), "equal_to_checker": bool(same)}
    assert r._lib.fs_host_unregister(host.ctypes.data) == 0
    print(json.dumps(out), flush=True)


r = GPURenderer(0)
geometry(r, "C3", 3840, 2160, 1)
if not args.skip_c4:
    geometry(r, "C4", 3840, 2160, 4)
r.close()
