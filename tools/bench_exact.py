#!/usr/bin/env python3
"""The exact renderer (fs_render_exact) measured: the numbers of DESIGN.md 6.3.

  pace      per limb count L: microseconds per step of a wave whose 64 samples never escape, from the difference of two frames of
            8 waves (one per workgroup, so each has a compute unit's SIMD to itself) that differ in the cap only; and the chip-wide
            rate of 32 x 32 -> 64 multiply-adds with every SIMD full (a 1024 x 1024 frame of never-escaping samples; a step is
            2 L^2 + L multiply-adds: two squares of L (L + 1) / 2 each and one product of L^2)
  frames    View 0 at 1024 x 768 (R 4), shallow_1e-28 at 1920 x 1080 (R 256) and View 5 at 1920 x 1080 (R 256; --view5, minutes),
            each with the share of lane slots spent on finished lanes with and without the compaction, and against the GMP counter on 16
            threads: the counter is timed on a lattice of the frame's samples and SCALED to the frame's sample count
  c3        (with --view5) how many pixels of the HDRFloat<float> LAv2 frame of View 5 at 1920 x 1080 differ from the exact frame: a
            recorded characterisation, not a test

  wide      (--wide) the one-wave-per-sample kernel (fs_exact_sample_counts) per limb count of --wide-limbs: microseconds per step
            of a lone wave (8 never-escaping samples, two caps apart, the difference) and the chip's pace with 1 024, 2 048 and
            4 096 such samples, as steps per second and as multiply-adds per second: `executed` counts what the lanes issue
            (3 products of ceil(L / M) rounds of M^2 in each of 64 lanes, M = ceil(L / 64)), `useful` the 2 L^2 + L of the narrow
            kernel's count, the figure to put next to its 9.0e12
  view11    (--view11) View 11's 200 fixture samples at the fixture's cap, (--view14) View 14's six at cap 1 800 000: equality with
            the fixture's counts and the wall time next to the entry's generator_seconds.  One run each.

  cycle     (--cycle) the cycle check (fs_set_exact_cycle_check; DESIGN.md 6.3 "Cycle check"): (a) what it costs where it proves
            nothing -- the two paces of `pace`, with the check off and on in the same run, on frames whose every sample is c = 1/4 (a
            parabolic point: never escapes, never repeats; the tool asserts that no sample was proved), per limb count of
            --cycle-limbs, as the on / off ratio of the time per step; (b) what it saves: View 0 at 1024 x 768 (R 4) with the check
            off and on at caps 8 192 and 100 000: call time, launches, steps and proved samples

  continue  (--continue) the continuation (fs_set_exact_keep, fs_render_exact_continue; DESIGN.md 6.3 "Continuation"): View 0 at
            1024 x 768 (R 4), caps 8 192 -> 100 000, with the cycle check off and on, in one run: the first call with keep on NEXT TO
            the same call with keep off (what keeping costs: the park stores, the repack, the kept block); the continuation NEXT TO
            a fresh call at the larger cap (the saving); samples kept, device bytes held, steps and launches of each.  The frame after
            the continuation is asserted equal to the fresh one.  No gate.

Times are host clocks around synchronous calls.  One JSON line per measurement.

  python tools/bench_exact.py [--pace] [--frames] [--view5] [--limbs 2,4,7,8,11,12,16,20,23,24]
                              [--wide] [--wide-limbs 25,64,80,128,160,320,683,704] [--view11] [--view14]
                              [--cycle] [--cycle-limbs 2,4,8,12,16,24] [--continue]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fractalshark_amd import GPURenderer, LAV2_FULL, PARITY_CPU, T_HDR32, exact, inputs  # noqa: E402
import _truth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pace", action="store_true")
ap.add_argument("--frames", action="store_true")
ap.add_argument("--view5", action="store_true")
ap.add_argument("--limbs", default="2,4,7,8,11,12,16,20,23,24")
ap.add_argument("--wide", action="store_true")
ap.add_argument("--wide-limbs", default="25,64,80,128,160,320,683,704")
ap.add_argument("--view11", action="store_true")
ap.add_argument("--view14", action="store_true")
ap.add_argument("--cycle", action="store_true")
ap.add_argument("--cycle-limbs", default="2,4,8,12,16,24")
ap.add_argument("--continue", dest="cont", action="store_true")
args = ap.parse_args()
if not (args.pace or args.frames or args.view5 or args.wide or args.view11 or args.view14 or args.cycle or args.cont):
    args.pace = args.frames = True


def say(**kw):
    print(json.dumps(kw), flush=True)


def inside_axes(L, w, h, F):
    """Axes of a w x h frame around c = -0.1 + 0.1i (inside the main cardioid: no sample ever escapes), spacing 2^-30."""
    val = lambda q, i: (int(q * (1 << 40)) << (F - 40)) + (i << (F - 30))
    limbs = lambda v: [(v >> (32 * l)) & 0xFFFFFFFF for l in range(L)]
    cx = np.array([limbs(val(-0.1, i)) for i in range(w)], np.uint32).T.copy()
    cy = np.array([limbs(val(0.1, i)) for i in range(h)], np.uint32).T.copy()
    return cx, cy


def quarter_axes(L, w, h, F):
    """Axes of a w x h frame whose every sample is c = 1/4: it creeps towards 1/2 for ever, so it neither escapes nor repeats."""
    limbs = lambda v: [(v >> (32 * l)) & 0xFFFFFFFF for l in range(L)]
    cx = np.array([limbs(1 << (F - 2))] * w, np.uint32).T.copy()
    return cx, np.zeros((L, h), np.uint32)


def timed_render(r, F, L, cx, cy, R, n):
    t0 = time.perf_counter()
    err = r.RenderExact(4, F, L, cx, cy, R, False, n)
    dt = time.perf_counter() - t0
    assert err == 0, err
    return dt


r = GPURenderer(0)

def pace(L, F, make_axes):
    """(microseconds per step of a wave by itself, lane steps per second of the full chip) on frames of make_axes' samples."""
    # eight waves, one per workgroup
    assert r.InitializeMemory(64, 8, 1, None, 0, 0, 0, False) == 0
    cx, cy = make_axes(L, 64, 8, F)
    n1, n2 = 4096, 4096 * 9
    timed_render(r, F, L, cx, cy, 4, n1)
    t1 = min(timed_render(r, F, L, cx, cy, 4, n1) for _ in range(3))
    t2 = min(timed_render(r, F, L, cx, cy, 4, n2) for _ in range(3))
    us_step = (t2 - t1) / (n2 - n1) * 1e6
    # every SIMD full
    assert r.InitializeMemory(1024, 1024, 1, None, 0, 0, 0, False) == 0
    cx, cy = make_axes(L, 1024, 1024, F)
    m1, m2 = 64, 64 + (512 if L <= 12 else 128)
    timed_render(r, F, L, cx, cy, 4, m1)
    u1 = min(timed_render(r, F, L, cx, cy, 4, m1) for _ in range(2))
    u2 = min(timed_render(r, F, L, cx, cy, 4, m2) for _ in range(2))
    return us_step, (m2 - m1) * 1024 * 1024 / (u2 - u1)


if args.pace:
    r.SetExactSlice(4096)  # (the default shortens the slices of a frame that fills the chip)
    for L in [int(s) for s in args.limbs.split(",")]:
        F = 32 * L - 10
        us_step, lane_steps = pace(L, F, inside_axes)
        say(what="pace", limbs=L, frac_bits=F, wave_us_per_step=round(us_step, 4), slice_of_4096_ms=round(us_step * 4096 / 1000, 2),
            chip_lane_steps_per_s=round(lane_steps), chip_gmad_per_s=round(lane_steps * (2 * L * L + L) / 1e9, 1))


if args.cycle:
    r.SetExactSlice(4096)
    for L in [int(s) for s in args.cycle_limbs.split(",")]:
        F = 32 * L - 10
        got = {}
        for on in (False, True):
            assert r.SetExactCycleCheck(on) == 0
            got[on] = pace(L, F, quarter_axes)
            assert r.exact_cycle_stats()[0] == 0 and r.exact_stats()["lane_steps"] > 0  # nothing proved: the two paces compare
        r.SetExactCycleCheck(False)
        say(what="cycle pace", limbs=L, frac_bits=F, wave_us_per_step_off=round(got[False][0], 4),
            wave_us_per_step_on=round(got[True][0], 4), wave_on_over_off=round(got[True][0] / got[False][0], 3),
            chip_lane_steps_per_s_off=round(got[False][1]), chip_lane_steps_per_s_on=round(got[True][1]),
            chip_on_over_off=round(got[False][1] / got[True][1], 3))
    r.SetExactSlice(0)
    c = _truth.Case("view0_1024x768")
    v, F = c.view(inputs), c.raw["frac_bits"]
    L = exact.limbs_for(F)
    cx, cy = exact.axes(v, F, limbs=L)
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0
    for cap in (8192, 100000):
        row, frames = {}, {}
        for on in (False, True):
            assert r.SetExactCycleCheck(on) == 0
            timed_render(r, F, L, cx, cy, 4, 64)  # (memory and code warm)
            dt = timed_render(r, F, L, cx, cy, 4, cap)
            st = r.exact_stats()
            row["on" if on else "off"] = dict(seconds=round(dt, 4), launches=st["launches"], lane_steps=st["lane_steps"],
                                              lane_slots=st["lane_slots"], proved=r.exact_cycle_stats()[0],
                                              checkpoint_reads=r.exact_cycle_stats()[1])
            frames[on] = r.new_iter_buffer()
            assert r.RenderCurrent(cap, frames[on]) == 0 and r.SyncComputeStream() == 0
        r.SetExactCycleCheck(False)
        assert frames[True].tobytes() == frames[False].tobytes()
        say(what="cycle frame", name="view0_1024x768", bailout=4, frac_bits=F, limbs=L, cap=cap,
            at_the_cap=int((frames[True][:c.h, :c.w] == cap).sum()), **row,
            time_off_over_on=round(row["off"]["seconds"] / row["on"]["seconds"], 2))

if args.cont:
    r.SetExactSlice(0)
    c = _truth.Case("view0_1024x768")
    v, F = c.view(inputs), c.raw["frac_bits"]
    L = exact.limbs_for(F)
    cx, cy = exact.axes(v, F, limbs=L)
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0
    n1, n2 = 8192, 100000

    def grab(cap):
        out = r.new_iter_buffer()
        assert r.RenderCurrent(cap, out) == 0 and r.SyncComputeStream() == 0
        return out

    def work(dt):
        st = r.exact_stats()
        return dict(seconds=round(dt, 4), launches=st["launches"], lane_steps=st["lane_steps"], proved=r.exact_cycle_stats()[0])

    for on in (False, True):
        assert r.SetExactCycleCheck(on) == 0 and r.SetExactKeep(False) == 0
        timed_render(r, F, L, cx, cy, 4, 64)  # (memory and code warm)
        row = {"first_keep_off": work(timed_render(r, F, L, cx, cy, 4, n1))}
        row["fresh_at_larger_cap"] = work(timed_render(r, F, L, cx, cy, 4, n2))
        fresh = grab(n2)
        assert r.SetExactKeep(True) == 0
        row["first_keep_on"] = work(timed_render(r, F, L, cx, cy, 4, n1))
        kept = r.ExactKept()
        t0 = time.perf_counter()
        err = r.RenderExactContinue(n2)
        row["continuation"] = work(time.perf_counter() - t0)
        assert err == 0 and grab(n2).tobytes() == fresh.tobytes()
        assert r.SetExactKeep(False) == 0 and r.DropExactKept() == 0
        say(what="continue", name="view0_1024x768", bailout=4, frac_bits=F, limbs=L, caps=[n1, n2], cycle_check=on,
            kept_samples=kept["samples"], kept_proved=kept["proved"], kept_device_bytes=kept["device_bytes"], **row,
            keep_on_over_keep_off_first_call=round(row["first_keep_on"]["seconds"] / row["first_keep_off"]["seconds"], 3),
            fresh_over_continuation=round(row["fresh_at_larger_cap"]["seconds"] / row["continuation"]["seconds"], 2))
    r.SetExactCycleCheck(False)

r.SetExactSlice(0)


def timed_counts(r, F, L, cx, cy, n):
    t0 = time.perf_counter()
    err, out = r.ExactSampleCounts(F, L, cx, cy, 4, False, n)
    dt = time.perf_counter() - t0
    assert err == 0 and (out == n).all(), err
    return dt


if args.wide:
    r.SetExactSlice(1 << 20)  # (one launch per call: the caps below are far under it)
    for L in [int(s) for s in args.wide_limbs.split(",")]:
        F = 32 * L - 10
        M = (L + 63) // 64
        nb = (L + M - 1) // M
        d = int(min(20000, max(300, 3e7 / (L * L))))
        n1, n2 = d // 4, d // 4 + d
        cx, cy = inside_axes(L, 8, 8, F)
        timed_counts(r, F, L, cx, cy, n1)
        t1 = min(timed_counts(r, F, L, cx, cy, n1) for _ in range(3))
        t2 = min(timed_counts(r, F, L, cx, cy, n2) for _ in range(3))
        us_step = (t2 - t1) / d * 1e6
        row = dict(what="wide", limbs=L, frac_bits=F, limbs_per_lane=M, rounds=nb, wave_us_per_step=round(us_step, 3),
                   steps_in_50_ms=int(50e3 / us_step))
        for n in (1024, 2048, 4096):
            cx, cy = inside_axes(L, n, n, F)
            timed_counts(r, F, L, cx, cy, n1)
            u1 = min(timed_counts(r, F, L, cx, cy, n1) for _ in range(2))
            u2 = min(timed_counts(r, F, L, cx, cy, n2) for _ in range(2))
            steps = n * d / (u2 - u1)
            row["chip_%d" % n] = dict(steps_per_s=round(steps), executed_gmad_per_s=round(steps * 3 * 64 * nb * M * M / 1e9, 1),
                                      useful_gmad_per_s=round(steps * (2 * L * L + L) / 1e9, 1))
        say(**row)
    r.SetExactSlice(0)

for flag, name, cap in ((args.view11, "view11_64x36", None), (args.view14, "view14_15360x8640_attempt", 1800000)):
    if not flag:
        continue
    c = _truth.Case(name)
    v, F = c.view(inputs), c.raw["frac_bits"]
    cap = c.cap if cap is None else cap
    v.num_iterations = cap
    t0 = time.perf_counter()
    values, _ = exact.sample_counts(r, v, c.xs, c.ys, bailout=256, frac_bits=F)
    dt = time.perf_counter() - t0
    want = _truth.expect_minus_one(c.counts(256), cap)
    st = r.exact_stats()
    say(what="fixture samples", name=name, frac_bits=F, limbs=exact.limbs_for(F), samples=len(c.xs), cap=cap, seconds=round(dt, 2),
        differ=int((values != want).sum()), steps=st["lane_steps"], launches=st["launches"],
        generator_seconds=c.raw["generator_seconds"], speedup_vs_generator=round(c.raw["generator_seconds"] / dt, 1))


def gmp_seconds(v, w, h, R, F, cap, cols, rows):
    """The GMP counter (16 threads) on a cols x rows lattice of the frame, and that time scaled to all w * h samples."""
    xs, ys = _truth.lattice(w, h, cols, rows)
    t0 = time.perf_counter()
    _truth.exact_counts(v.bbox(), w, h, xs, ys, cap + 1, R, F, shifts=[])
    dt = time.perf_counter() - t0
    return dt, len(xs), dt * w * h / len(xs)


def frame(name, v, w, h, R, F, cap, lattice, both_modes=True):
    v.num_iterations = cap
    L = exact.limbs_for(F)
    cx, cy = exact.axes(v, F, limbs=L)
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False) == 0
    out = {}
    for mode in (("compaction", "no_compaction") if both_modes else ("compaction",)):
        r.SetExactSlice(0, no_compaction=mode == "no_compaction")
        timed_render(r, F, L, cx, cy, R, min(cap, 64))  # (memory and code warm)
        dt = timed_render(r, F, L, cx, cy, R, cap)
        st = r.exact_stats()
        out[mode] = dict(seconds=round(dt, 4), launches=st["launches"], lane_steps=st["lane_steps"], lane_slots=st["lane_slots"],
                         finished_lane_share=round(1 - st["lane_steps"] / max(1, st["lane_slots"]), 4))
    r.SetExactSlice(0)
    g_dt, g_n, g_scaled = gmp_seconds(v, w, h, R, F, cap, *lattice)
    say(what="frame", name=name, width=w, height=h, bailout=R, frac_bits=F, limbs=L, cap=cap, **out,
        gmp16_lattice_samples=g_n, gmp16_lattice_seconds=round(g_dt, 3), gmp16_scaled_to_frame_seconds=round(g_scaled, 1),
        speedup_vs_scaled_gmp16=round(g_scaled / out["compaction"]["seconds"], 1))


if args.frames:
    c = _truth.Case("view0_1024x768")
    frame("view0_1024x768", c.view(inputs), c.w, c.h, 4, c.raw["frac_bits"], c.cap, (64, 48))
    c = _truth.Case("shallow_1e-28")
    b = c.raw["bbox"]
    v = inputs.View(b[0], b[1], b[2], b[3], 1920, 1080, num_iterations=c.cap)
    frame("shallow_1e-28 at 1920x1080", v, 1920, 1080, 256, v.precision_bits + exact.GUARD_BITS, c.cap, (64, 36))

if args.view5:
    c = _truth.Case("view5_1920x1080")
    v = c.view(inputs)
    F = c.raw["frac_bits"]
    frame("view5_1920x1080", v, c.w, c.h, 256, F, c.cap, (12, 8), both_modes=False)
    ex = r.new_iter_buffer()
    assert r.RenderCurrent(c.cap, ex) == 0 and r.SyncComputeStream() == 0
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    assert r.InitializePerturb(1, ob, 0, None, la) == 0
    co = [(float(k["m"]), int(k["e"])) for k in v.coords_perturb_hdr32(ob)]
    assert r.RenderPerturbLAv2(None, None, None, *co, c.cap, T=T_HDR32, Mode=LAV2_FULL, parity=PARITY_CPU) == 0
    got = r.new_iter_buffer()
    assert r.RenderCurrent(c.cap, got) == 0 and r.SyncComputeStream() == 0
    diff = got[:c.h, :c.w].astype(np.int64) - ex[:c.h, :c.w].astype(np.int64)
    say(what="c3", name="view5_1920x1080 HDRFloat<float> LAv2 against the exact frame", pixels=int(diff.size),
        differ=int((diff != 0).sum()), differ_by_more_than_one=int((np.abs(diff) > 1).sum()), largest=int(np.abs(diff).max()))

r.close()
