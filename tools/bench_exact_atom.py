#!/usr/bin/env python3
"""What the exact renderer's period planes (fs_set_exact_periods; DESIGN.md 6.3 "Period planes") cost, on one MI355X.

  pace     the two paces of DESIGN.md 6.3's table -- a lone wave's microseconds per step and the full chip's lane steps per second,
           measured as tools/bench_exact.py measures them -- with the switch off and on in the same run, on frames whose every
           sample is c = 1/4: it never escapes, and its smallest norm is the first, so the switch-on kernel does its per-step work
           (the key of every norm, one 64-bit compare) and never takes a new minimum after n = 1.  The switch-off kernels are the
           ones of the parent's table: their pace must match it within its 2-3 % box-to-box spread.
  view5    exact.render_periods of View 5 at 64 x 36 (the fixture's view5_64x36: cap 4.7 million, F = 331, 11 limbs) against
           exact.render of the same frame: the two call times, the frames compared byte for byte, and how many of the 2 304 pixels
           carry atom period 60 030, the view's period -- a finding, not an assertion.

Host clock around the synchronous calls, best of two or three after a warm-up; one JSON line per measurement.

  python tools/bench_exact_atom.py [--pace] [--view5] [--limbs 2,8,16,24]
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
from fractalshark_amd import GPURenderer, exact, inputs  # noqa: E402
import _truth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pace", action="store_true")
ap.add_argument("--view5", action="store_true")
ap.add_argument("--limbs", default="2,8,16,24")
args = ap.parse_args()
if not (args.pace or args.view5):
    args.pace = args.view5 = True

VIEW5_PERIOD = 60030


def say(**kw):
    print(json.dumps(kw), flush=True)


def quarter_axes(L, w, h, F):
    """Axes of a w x h frame whose every sample is c = 1/4."""
    limbs = lambda v: [(v >> (32 * l)) & 0xFFFFFFFF for l in range(L)]
    cx = np.array([limbs(1 << (F - 2))] * w, np.uint32).T.copy()
    return cx, np.zeros((L, h), np.uint32)


def timed_render(r, F, L, cx, cy, n):
    t0 = time.perf_counter()
    err = r.RenderExact(4, F, L, cx, cy, 4, False, n)
    dt = time.perf_counter() - t0
    assert err == 0, err
    return dt


r = GPURenderer(0)


def pace(L, F):
    """(microseconds per step of a wave by itself, lane steps per second of the full chip): tools/bench_exact.py's measurement."""
    assert r.InitializeMemory(64, 8, 1, None, 0, 0, 0, False) == 0
    cx, cy = quarter_axes(L, 64, 8, F)
    n1, n2 = 4096, 4096 * 9
    timed_render(r, F, L, cx, cy, n1)
    t1 = min(timed_render(r, F, L, cx, cy, n1) for _ in range(3))
    t2 = min(timed_render(r, F, L, cx, cy, n2) for _ in range(3))
    us_step = (t2 - t1) / (n2 - n1) * 1e6
    assert r.InitializeMemory(1024, 1024, 1, None, 0, 0, 0, False) == 0
    cx, cy = quarter_axes(L, 1024, 1024, F)
    m1, m2 = 64, 64 + (512 if L <= 12 else 128)
    timed_render(r, F, L, cx, cy, m1)
    u1 = min(timed_render(r, F, L, cx, cy, m1) for _ in range(2))
    u2 = min(timed_render(r, F, L, cx, cy, m2) for _ in range(2))
    return us_step, (m2 - m1) * 1024 * 1024 / (u2 - u1)


if args.pace:
    r.SetExactSlice(4096)
    for L in [int(s) for s in args.limbs.split(",")]:
        F = 32 * L - 10
        got = {}
        for on in (False, True):
            assert r.SetExactPeriods(on) == 0
            got[on] = pace(L, F)
            if on:  # (the last frame: 1024 x 1024 samples of c = 1/4, every one with its smallest norm at n = 1)
                err, atom = r.ExactAtomPeriods()
                assert err == 0 and bool((atom == 1).all())
        r.SetExactPeriods(False)
        say(what="periods pace", limbs=L, frac_bits=F, wave_us_per_step_off=round(got[False][0], 4),
            wave_us_per_step_on=round(got[True][0], 4), wave_on_over_off=round(got[True][0] / got[False][0], 3),
            chip_lane_steps_per_s_off=round(got[False][1]), chip_lane_steps_per_s_on=round(got[True][1]),
            chip_on_over_off=round(got[False][1] / got[True][1], 3))
    r.SetExactSlice(0)

if args.view5:
    c = _truth.Case("view5_64x36")
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0 and r.ClearMemory() == 0
    t0 = time.perf_counter()
    exact.render(r, v, bailout=256, frac_bits=F)
    t_plain = time.perf_counter() - t0
    plain = r.new_iter_buffer()
    assert r.RenderCurrent(c.cap, plain) == 0 and r.SyncComputeStream() == 0
    assert r.ClearMemory() == 0
    t0 = time.perf_counter()
    frame, atom = exact.render_periods(r, v, bailout=256, frac_bits=F)
    t_periods = time.perf_counter() - t0  # (includes reading the frame and the plane back)
    periods, counts = np.unique(atom, return_counts=True)
    top = sorted(zip(counts.tolist(), periods.tolist()), reverse=True)[:8]
    say(what="view5_64x36", limbs=exact.limbs_for(F), frac_bits=F, cap=c.cap, render_s=round(t_plain, 2),
        render_periods_s=round(t_periods, 2), periods_over_plain=round(t_periods / t_plain, 3),
        frames_equal=bool(frame.tobytes() == plain[:c.h, :c.w].tobytes()), pixels=int(atom.size),
        pixels_with_atom_period_60030=int((atom == VIEW5_PERIOD).sum()),
        pixels_with_a_multiple_of_60030=int(((atom % VIEW5_PERIOD == 0) & (atom != 0)).sum()),
        commonest_atom_periods=[[p, n] for n, p in top])

r.close()
