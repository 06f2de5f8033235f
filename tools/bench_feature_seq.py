#!/usr/bin/env python3
"""Times of the Feature Finder's PT evaluator on a waypoint-resident orbit (fs_feature_eval_resident) for DESIGN.md section 6.1.
One process, View 5 (192 x 108 window), the same SimpleCompression orbit uploaded to two renderers: E expanded
(fs_set_compressed_orbit_mode 0, through fs_feature_eval) and S as waypoints only (mode 1).  For HDRFloat<float> and
HDRFloat<double>: the 12 x 12 scan at the view's iteration cap, and one wave's fixed-period step pace (64 lanes in lockstep on one
found candidate, PT only: the time at its period minus the time at a fourth of it, per step).  E in the same run is the
yardstick.  Prints one JSON line.  Usage: python tools/bench_feature_seq.py [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fractalshark_amd import GPURenderer, T_HDR32, T_HDR64, features, inputs  # noqa: E402

GRID = 12
# compression_exp per type: the waypoints are a ninth (HDRFloat<float>) / a hundredth (HDRFloat<double>) of the entries
COMPRESSION = {T_HDR32: 12, T_HDR64: 20}


def timed(f, repeats):
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def renderer_for(orbit, waypoints):
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
    assert r.set_compressed_orbit_mode(waypoints) == 0
    assert r.InitializePerturb(1, orbit) == 0
    assert r.orbit_form == (2 if waypoints else 1)
    return r


def search_round(view, orbit, cap):
    """(radius, records) of the scan's period-search round."""
    recs = []

    def grab(mode, radius, c, rin, rout):
        recs.append((radius.copy(), rin.copy()))
        rout["status"] = features.REJECTED  # ends the scan after its first round

    features.scan(view, orbit, grab, GRID, GRID, 4, cap)
    return recs[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    res = {}
    for T, name in ((T_HDR32, "hdr32"), (T_HDR64, "hdr64")):
        is64 = T == T_HDR64
        v = inputs.View.builtin(5, 192, 108)
        cap = v.num_iterations
        ob = inputs.Orbit(v, is64=is64, compression_exp=COMPRESSION[T])
        E, S = renderer_for(ob, False), renderer_for(ob, True)
        _, dout, _ = features.records(is64)
        radius, rin = search_round(v, ob, cap)
        first = np.zeros(len(rin), dout)
        entry = {"E": E.FeatureEval, "S": S.FeatureEvalResident}
        for r in entry.values():  # (first launches: code load)
            assert r(T, 4, features.FIND, radius, 64, rin, first) == 0
        assert E.FeatureEval(T, 4, features.FIND, radius, cap, rin, first) == 0
        ok = np.nonzero(first["status"] == features.OK)[0]
        k = ok[np.argsort(first["period"][ok])[len(ok) // 2]]  # a candidate of the median period
        p = int(first["period"][k])
        lanes = np.repeat(rin[k:k + 1], 64)
        out = {"cap": cap, "entries": int(ob.count), "waypoints": int(ob.compressed_count), "wave_period": p}
        for form, r in (("E", E), ("S", S)):
            ts = []
            for steps in (p // 4, p):  # (a fixed-period evaluation runs that many steps, periodic or not)
                lanes["period"] = steps
                rout = np.zeros(64, dout)
                t, err = timed(lambda: entry[form](T, 4, features.FIXED, radius, cap, lanes, rout), a.repeats)
                assert err == 0 and (rout["status"] == features.OK).all(), "not PT only: %s" % (rout["status"][:4],)
                ts.append(t)
            t_scan, found = timed(lambda: features.find_periodic_points(r, v, ob, GRID, GRID, T, 4, cap), a.repeats)
            t_find, _ = timed(lambda: entry[form](T, 4, features.FIND, radius, cap, rin, np.zeros(len(rin), dout)), a.repeats)
            out[form] = {"orbit_device_bytes": r.orbit_device_bytes, "wave_step_ns": round((ts[1] - ts[0]) / (p - p // 4) * 1e9, 1),
                         "scan12_s": round(t_scan, 4), "search_round_s": round(t_find, 4), "found": len(found)}
            out[form + "_found"] = found
        assert out.pop("E_found") == out.pop("S_found")
        out["step_ratio_S_over_E"] = round(out["S"]["wave_step_ns"] / out["E"]["wave_step_ns"], 3)
        out["scan_ratio_S_over_E"] = round(out["S"]["scan12_s"] / out["E"]["scan12_s"], 3)
        res[name] = out
        E.close()
        S.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
