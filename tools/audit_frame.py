#!/usr/bin/env python3
"""Render a named workload's frame and ask the library which sample pixels are wrong (exact.audit, fs_exact_audit).

A workload is CASE:KERNEL.  CASE is a case of the exact-count fixture (tests/golden/exact_counts.json: its view, size and cap --
shallow_1e-28, view5_3840x2160, ...); KERNEL is hdr32 or hdr64 (LAv2 Full in HDRFloat<float> / HDRFloat<double>) or exact (the
exact renderer itself: an audit of it must find nothing).  c3_hdr32 and c3_hdr64 are view5_3840x2160:hdr32 / :hdr64, the frame of
bench.py's c3_lav2 in the two mantissa widths.  The lattice defaults to the fixture's own for the case, the levels to its ladder.

One JSON line per audit: the record per level (stable, stable_differ, stable_capped, max_abs_diff), the finest clean level, the
first offenders, and the time of the audit call (a host clock around exact.audit: the axes on the host, all runs, the
classification, the read-back of the record).  --against-sample-counts also runs exact.sample_counts -- one synchronous call per
run position, a wave per sample -- on the same samples and levels in the same process, checks that both agree and prints the
factor between the two times.  --prove-interior audits with the cycle check on (exact.audit(prove_interior=True), DESIGN.md 6.3
"Cycle check"; up to 24 limbs): the record must be the same, and the line also carries n_proved (of the samples' own runs),
runs_proved (of all runs) and the checkpoints read back.  One run each; the first call of either path in a process is preceded by a two-sample call that
loads its kernels.

  python tools/audit_frame.py shallow_1e-28:exact --against-sample-counts
  python tools/audit_frame.py c3_hdr32 c3_hdr64 --levels 17,30 [--parity cpu|gpustage] [--lattice 24x12]
  python tools/audit_frame.py view0_70x37:exact --prove-interior
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
from fractalshark_amd import (GPURenderer, LAV2_FULL, PARITY_CPU, PARITY_CPU_GPUSTAGE, T_HDR32, T_HDR64, exact,  # noqa: E402
                              inputs)
import _truth  # noqa: E402

ALIASES = {"c3_hdr32": "view5_3840x2160:hdr32", "c3_hdr64": "view5_3840x2160:hdr64"}

ap = argparse.ArgumentParser()
ap.add_argument("workloads", nargs="+")
ap.add_argument("--levels", default=None, help="comma-separated ladder levels (at most 8); default: the case's ladder")
ap.add_argument("--lattice", default=None, help="COLSxROWS over the frame; default: the fixture's samples of the case")
ap.add_argument("--parity", choices=("cpu", "gpustage"), default="cpu", help="stage-test direction of the LAv2 kernels")
ap.add_argument("--against-sample-counts", action="store_true")
ap.add_argument("--prove-interior", action="store_true", help="audit with the exact renderer's cycle check on")
args = ap.parse_args()


def render(r, c, v, kernel, F):
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0 and r.ClearMemory() == 0
    t0 = time.perf_counter()
    if kernel == "exact":
        exact.render(r, v, bailout=256, frac_bits=F)
    else:
        ob = inputs.Orbit(v, is64=kernel == "hdr64")
        assert r.InitializePerturb(1, ob, 0, None, inputs.LATable(ob)) == 0
        co = [(float(k["m"]), int(k["e"])) for k in v.coords_perturb(ob)]
        assert r.RenderPerturbLAv2(None, None, None, *co, c.cap, T=T_HDR64 if kernel == "hdr64" else T_HDR32, Mode=LAV2_FULL,
                                   parity=PARITY_CPU if args.parity == "cpu" else PARITY_CPU_GPUSTAGE) == 0
    assert r.SyncComputeStream() == 0
    return time.perf_counter() - t0


r = GPURenderer(0)
for wl in args.workloads:
    name, _, kernel = ALIASES.get(wl, wl).partition(":")
    kernel = kernel or "hdr32"
    assert kernel in ("hdr32", "hdr64", "exact"), kernel
    c = _truth.Case(name)
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    levels = tuple(int(s) for s in args.levels.split(",")) if args.levels else c.ladder
    if args.lattice:
        cols, rows = (int(s) for s in args.lattice.split("x"))
        xs, ys = exact.lattice(v, cols, rows)
    else:
        xs, ys = c.xs, c.ys
    render_s = render(r, c, v, kernel, F)
    exact.audit(r, v, xs[:2], ys[:2], levels=(), bailout=256, frac_bits=F)  # (loads the kernels)
    t0 = time.perf_counter()
    rep = exact.audit(r, v, xs, ys, levels=levels, bailout=256, frac_bits=F, prove_interior=args.prove_interior)
    audit_s = time.perf_counter() - t0
    st = r.exact_stats()
    line = dict(what="audit", workload=wl, case=name, kernel=kernel, parity=args.parity if kernel != "exact" else None,
                width=c.w, height=c.h, cap=c.cap, frac_bits=F, limbs=exact.limbs_for(F), samples=len(xs),
                runs=len(xs) * (1 + 4 * len(levels)), **rep.as_dict(), finest_clean_level=rep.finest_clean_level(),
                offenders=rep.offenders[:4], render_seconds=round(render_s, 3), audit_seconds=round(audit_s, 4),
                launches=st["launches"], lane_steps=st["lane_steps"], lane_slots=st["lane_slots"])
    if args.prove_interior:
        runs_proved, compares = r.exact_cycle_stats()
        line.update(prove_interior=rep.proved is not None, n_proved=rep.n_proved, runs_proved=runs_proved, checkpoint_reads=compares)
    if args.against_sample_counts:
        exact.sample_counts(r, v, xs[:2], ys[:2], bailout=256, frac_bits=F)
        t0 = time.perf_counter()
        values, stable = exact.sample_counts(r, v, xs, ys, bailout=256, frac_bits=F, levels=levels)
        sc_s = time.perf_counter() - t0
        line.update(sample_counts_seconds=round(sc_s, 4), sample_counts_calls=1 + 4 * len(levels),
                    sample_counts_agrees=bool(np.array_equal(values, rep.values) and np.array_equal(stable, rep.stable)),
                    factor=round(sc_s / audit_s, 1))
    print(json.dumps(line), flush=True)
r.close()
