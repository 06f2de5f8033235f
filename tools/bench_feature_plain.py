#!/usr/bin/env python3
"""Times of the Feature Finder's plain-type evaluators (fs_feature_eval_plain, fs_feature_eval_plain_direct) for DESIGN.md section
6.1 "Plain types".  One process, best of --repeats after a warm-up call of each entry:
  wave   one wave's fixed-period PT step at the fixture view shallow_1e-20 (tests/_truth.py), 64 lanes in lockstep on one candidate
         the double period search accepts: the time at m periods minus the time at a fourth of them, per step (a fixed-period
         evaluation runs that many steps; m = 16, or fewer where the candidate escapes before); float and double on the expanded (E) and the waypoint-resident (S) orbit, next to HDRFloat<float> /
         HDRFloat<double> through fs_feature_eval on the same view and grid point;
  scans  the 12 x 12 and the 128 x 128 scan of shallow_1e-12 on the GPU and through the checker
         (tests/feature/feature_plain_ref.cpp) on 1 and 16 threads;
  direct the 1 024 x 1 024 period_map of View 0 at cap 8 192.
Prints one JSON line.  Usage: python tools/bench_feature_plain.py [--repeats 3] [--skip-dense]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _truth  # noqa: E402
from fractalshark_amd import GPURenderer, T_F32, T_F64, T_HDR32, T_HDR64, features, inputs  # noqa: E402
from test_feature_plain_cpu import WAYPOINT_EXP, checker_evaluator  # noqa: E402

CAP = 20000
TAG = {"f32": T_F32, "f64": T_F64}
# SimpleCompression exponents for the 8 111-entry orbit of shallow_1e-20
WAVE_EXP = {"f32": 6, "f64": 20}


def timed(f, repeats):
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def search_round(view, orbit, cap, grid=12):
    recs = []

    def grab(mode, radius, c, rin, rout):
        recs.append((radius.copy(), rin.copy()))
        rout["status"] = features.REJECTED  # ends the scan after its first round

    features.scan(view, orbit, grab, grid, grid, 4, cap)
    return recs[0]


def plain_renderer(p, waypoints):
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
    assert r.set_compressed_orbit_mode(waypoints) == 0
    assert r.InitializePerturbPlain(1, p, with_la=False) == 0
    assert r.orbit_form == (2 if waypoints else 1)
    return r


def wave_pace(entry, T, radius, rec, dout, period, repeats):
    """(ns per step, m) of 64 copies of `rec`, PT only: the time at m periods minus the time at a fourth of them, per step, for
    the largest m of 16, 4, 1 at which the evaluation stays in PT (a candidate off the nucleus may escape after some periods)."""
    lanes = np.repeat(rec, 64)
    for m in (16, 4, 1):
        ts = []
        for steps in (m * period // 4, m * period):
            lanes["period"] = steps
            rout = np.zeros(64, dout)
            assert entry(T, 4, features.FIXED, radius, CAP, lanes, rout) == 0  # warm-up
            t, err = timed(lambda: entry(T, 4, features.FIXED, radius, CAP, lanes, rout), repeats)
            assert err == 0
            if not (rout["status"] == features.OK).all():
                break
            ts.append(t)
        if len(ts) == 2:
            return round((ts[1] - ts[0]) / (m * period - m * period // 4) * 1e9, 1), m
    raise AssertionError("not PT only at one period: %s" % (rout["status"][:4],))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-dense", action="store_true", help="leave out the 128 x 128 scan and the 1 024 x 1 024 map")
    a = ap.parse_args()
    res = {}

    # ---- one wave's step
    v = _truth.Case("shallow_1e-20").view(inputs)
    p64 = inputs.PlainInputs(v, "f64", max_iter=CAP)
    radius, rin = search_round(v, p64, CAP)
    first = np.zeros(len(rin), features.FEATURE_OUT_F64)
    checker_evaluator(p64, 4, threads=16)(features.FIND, radius, CAP, rin, first)
    ok = np.nonzero(first["status"] == features.OK)[0]
    k = int(ok[np.argsort(first["period"][ok])[len(ok) // 2]])  # a candidate of the median period
    period = int(first["period"][k])
    wave = {"view": "shallow_1e-20", "grid_point": k, "period": period, "entries": int(p64.count)}
    for kind in ("f32", "f64"):
        dout = features.records_plain(kind == "f64")[1]
        pc = inputs.PlainInputs(v, kind, max_iter=CAP, compression_exp=WAVE_EXP[kind])
        rad, recs = search_round(v, pc, CAP)
        wave[kind] = {"waypoints": int(pc.compressed_count)}
        for form, waypoints in (("E", False), ("S", True)):
            r = plain_renderer(pc, waypoints)
            ns, m = wave_pace(r.FeatureEvalPlain, TAG[kind], rad, recs[k:k + 1], dout, period, a.repeats)
            wave[kind][form + "_step_ns"], wave[kind][form + "_periods"] = ns, m
            r.close()
    for T, name in ((T_HDR32, "hdr32"), (T_HDR64, "hdr64")):
        ob = inputs.Orbit(v, is64=T == T_HDR64, max_iter=CAP)
        rad, recs = search_round(v, ob, CAP)
        r = GPURenderer(0)
        assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
        assert r.InitializePerturb(1, ob) == 0
        ns, m = wave_pace(r.FeatureEval, T, rad, recs[k:k + 1], features.records(T == T_HDR64)[1], period, a.repeats)
        wave[name] = {"E_step_ns": ns, "E_periods": m}
        r.close()
    wave["hdr32_over_f32"] = round(wave["hdr32"]["E_step_ns"] / wave["f32"]["E_step_ns"], 2)
    wave["hdr64_over_f64"] = round(wave["hdr64"]["E_step_ns"] / wave["f64"]["E_step_ns"], 2)
    res["wave"] = wave

    # ---- scans of shallow_1e-12
    v = _truth.Case("shallow_1e-12").view(inputs)
    scans = {}
    for kind in ("f32", "f64"):
        p = inputs.PlainInputs(v, kind, max_iter=CAP)
        r = plain_renderer(p, False)
        out = {"entries": int(p.count)}
        for grid in (12,) if a.skip_dense else (12, 128):
            features.find_periodic_points(r, v, p, 4, 4, TAG[kind], 4, CAP)  # warm-up
            t_gpu, found = timed(lambda: features.find_periodic_points(r, v, p, grid, grid, TAG[kind], 4, CAP), a.repeats)
            g = {"gpu_s": round(t_gpu, 4), "found": len(found)}
            for threads in (1, 16):
                t_cpu, want = timed(lambda: features.scan(v, p, checker_evaluator(p, 4, threads=threads), grid, grid, 4, CAP),
                                    a.repeats)
                assert want == found
                g["checker_%d_s" % threads] = round(t_cpu, 4)
            out["grid%d" % grid] = g
        pw = inputs.PlainInputs(v, kind, max_iter=CAP, compression_exp=WAYPOINT_EXP[kind])
        rw = plain_renderer(pw, True)
        features.find_periodic_points(rw, v, pw, 4, 4, TAG[kind], 4, CAP)
        t_s, found_s = timed(lambda: features.find_periodic_points(rw, v, pw, 12, 12, TAG[kind], 4, CAP), a.repeats)
        out["grid12_waypoints"] = {"gpu_s": round(t_s, 4), "found": len(found_s), "waypoints": int(pw.compressed_count)}
        rw.close()
        r.close()
        scans[kind] = out
    res["scans"] = scans

    # ---- Direct: the period map of View 0
    if not a.skip_dense:
        v0 = inputs.View.builtin(0, 1024, 1024)
        direct = {}
        for kind in ("f32", "f64"):
            r = GPURenderer(0)
            features.period_map(r, v0, 64, 64, T=TAG[kind], max_iters=8192)  # warm-up
            rin, rad = features.direct_grid(v0, kind == "f64", 1024, 1024, plain=True)
            rout = np.zeros(len(rin), features.records_plain(kind == "f64")[1])
            t_call, err = timed(lambda: r.FeatureEvalPlainDirect(TAG[kind], 4, features.FIND, rad, 8192, rin, rout), a.repeats)
            assert err == 0
            t_map, m = timed(lambda: features.period_map(r, v0, 1024, 1024, T=TAG[kind], max_iters=8192), a.repeats)
            direct[kind] = {"call_s": round(t_call, 4), "period_map_s": round(t_map, 4), "periods": int((m != 0).sum())}
            r.close()
        res["direct_1024"] = direct
    print(json.dumps(res))


if __name__ == "__main__":
    main()
