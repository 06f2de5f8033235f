#!/usr/bin/env python3
"""Exact escape counts of sampled pixels -> tests/golden/exact_counts.json (CPU only; minutes, the deep case tens of minutes).

For every case below: a lattice of sampled rows and columns across the whole frame; per sample the exact escape count from GMP
integer iteration at the view's precision plus a guard (tests/truth/exact_counts.cpp), and one stability bit per ladder level (the
count is unchanged when c moves by frame-width / 2^level in +x, -x, +y, -y).  Then each reference-pinned oracle path of the case
(tests/_truth.pinned_paths) is rendered at the sampled rows, and the finest level at which it equals the exact count's expected
value on every stable, uncapped sample is written next to it: the level at which unpinned paths of the same mantissa width and
mode are held to equality (tests/test_exact_counts.py, tests/test_gpu_exact_counts.py).

The guard is checked here: a subset of every case is recounted at twice the fractional bits and must give identical counts.

Data only is written: view number or bounding box, frame, cap, sampled rows / columns, counts, stability bits, levels.

  python tests/golden/make_exact_counts.py [--only shallow_1e-12,view0_1024x768,...]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(HERE, "exact_counts.json")

_X2_CENTRES = [("-0.5482057480704757084582125675467330293766992786373239", "-0.5775708389036038428051089822018505586755517268027721"),
               ("-1.7685736563152709932817429153295447129341", "0.0"),
               ("-0.1528465308235274786391493323577", "1.0397032701234428320367513768879")]


def generated_bbox(centre, width, W, H, prec):
    """The bounding box tests/test_plain_oracle.shallow_view (prec 60) and test_2x32_generated_views_* (prec 80) build."""
    from decimal import Decimal, getcontext
    getcontext().prec = prec
    cx, cy, w = Decimal(centre[0]), Decimal(centre[1]), Decimal(width)
    h = w * H / W
    return [str(cx - w / 2), str(cy - h / 2), str(cx + w / 2), str(cy + h / 2)]


def cases():
    import _truth
    P, D = _truth.PERTURB_KEYS, _truth.DIRECT_KEYS
    out = []
    for width in ("1e-6", "1e-12", "1e-20", "1e-28"):  # tests/test_plain_oracle.shallow_view
        out.append(dict(name="shallow_" + width, bbox=generated_bbox(_X2_CENTRES[0], width, 64, 36, 60), width=64, height=36,
                        cap=20000, cols=32, rows=18, R=[256, 4], pinned=P, scaled=True))
    for c in range(3):  # test_2x32_generated_views_full_and_perturbation_only
        for width in ("1e-8", "1e-14", "1e-22", "1e-31", "1e-40"):
            out.append(dict(name="x2_c%d_%s" % (c, width), bbox=generated_bbox(_X2_CENTRES[c], width, 48, 27, 80), width=48,
                            height=27, cap=30000, cols=24, rows=14, R=[256, 4], pinned=("m53_po", "m53_bla", "m53_lav2_gpustage"), hdr2x32=True))
    out.append(dict(name="view0_1024x768", view=0, width=1024, height=768, cap=8192, cols=33, rows=25, R=[4], pinned=D))
    out.append(dict(name="view0_70x37", view=0, width=70, height=37, cap=8192, cols=24, rows=19, R=[4], pinned=D))
    out.append(dict(name="view3_64x36", view=3, width=64, height=36, cap=None, cols=22, rows=12, R=[256], pinned=P, scaled=True))
    # View 9: HDRFloat<double> only.  HDRFloat<float>'s finest miss-free level there is 2^-17, where 46 of 264 samples are stable:
    # under both floors, so no 24-bit comparison rests on this case.
    out.append(dict(name="view9_64x36", view=9, width=64, height=36, cap=None, cols=22, rows=12, R=[256],
                    pinned=tuple(k for k in P if k.startswith("m53"))))
    out.append(dict(name="view5_64x36", view=5, width=64, height=36, cap=None, cols=32, rows=18, R=[256, 4],
                    pinned=P + ("m24_lav2_cpu_rc", "m53_lav2_cpu_rc"), scaled=True))
    out.append(dict(name="view5_1920x1080", view=5, width=1920, height=1080, cap=None, cols=24, rows=12, R=[256],
                    pinned=("m24_po", "m24_lav2_cpu", "m24_lav2_gpustage", "m53_po", "m53_lav2_gpustage")))
    out.append(dict(name="view5_3840x2160", view=5, width=3840, height=2160, cap=None, cols=24, rows=12, R=[256],
                    pinned=("m24_lav2_cpu", "m24_lav2_gpustage", "m53_lav2_cpu", "m53_lav2_gpustage")))
    # The deep cases.  View 19 at C5's frame: 2.6 - 2.9 million steps of 707-bit integers per orbit, so a cap just above the frame's
    # counts and a ladder without 2^-10 and 2^-22; HDRFloat<float> has no level there (listed with View 5's), the frame is held in
    # HDRFloat<double>.  (No m53_po: a 7680-wide row of 2.7-million-step pixels is hours of oracle per row.)
    out.append(dict(name="view19_7680x4320", view=19, width=7680, height=4320, cap=4000000, cols=20, rows=10, R=[256],
                    ladder=(12, 15, 17, 20, 25, 30, 35), pinned=("m24_bla", "m53_bla", "m53_lav2_cpu", "m53_lav2_gpustage")))
    # View 11 (2 486 bits, escapes at 0.5 million steps, 7 us a step): one level, the one Views 3 and 9 chose for HDRFloat<double> LAv2
    out.append(dict(name="view11_64x36", view=11, width=64, height=36, cap=None, cols=20, rows=10, R=[256], ladder=(25,), pinned=P))
    # View 14 at C4's frame and AA (15360 x 8640 samples), the cap the View 14 tests use: counts of six samples only, no stability
    # bits -- a measured attempt (seconds are in the entry), not a case a comparison rests on
    out.append(dict(name="view14_15360x8640_attempt", view=14, width=15360, height=8640, cap=1800000, cols=3, rows=2, R=[256],
                    ladder=(), pinned=(), attempt=True))
    return out


def build_case(spec, threads=16, log=print, reuse=None):
    """One fixture entry from a case specification (also what the CPU test regenerates for a small case).  reuse = an earlier
    entry of the same case whose counts are kept: only the levels and the recorded characterisations are made again."""
    import numpy as np

    import _truth
    from fractalshark_amd import inputs
    t0 = time.time()
    w, h = spec["width"], spec["height"]
    if "view" in spec:
        v = inputs.View.builtin(spec["view"], w, h, antialiasing=1)
        cap = spec["cap"] or v.num_iterations
    else:
        cap = spec["cap"]
        v = inputs.View(*spec["bbox"], w, h, num_iterations=cap)
    ladder = tuple(spec.get("ladder", _truth.LADDER))
    cols, rows = _truth.lattice_axes(w, h, spec["cols"], spec["rows"])
    gx, gy = np.meshgrid(cols, rows)
    xs, ys = gx.ravel(), gy.ravel()
    bbox, F = v.bbox(), v.precision_bits + _truth.GUARD_BITS
    entry = {"width": w, "height": h, "aa": 1, "cap": cap, "columns": cols.tolist(), "rows": rows.tolist(), "samples": len(xs),
             "ladder": list(ladder), "precision_bits": int(v.precision_bits), "frac_bits": int(F)}
    entry.update({"view": spec["view"]} if "view" in spec else {"bbox": spec["bbox"]})
    sub = np.arange(0, len(xs), max(1, len(xs) // 12))  # the guard check's subset
    exact = {}
    for R in spec["R"]:
        t1 = time.time()
        if reuse is not None:
            assert all(reuse[k] == entry[k] for k in ("columns", "rows", "cap", "ladder", "frac_bits")), spec["name"]
            rec = entry["R%d" % R] = reuse["R%d" % R]
            bits = np.array(rec["stable_bits"], np.int64)
            exact[R] = (np.array(rec["counts"], np.int64), ((bits[:, None] >> np.arange(len(ladder))) & 1).astype(bool))
            if not rec.get("guard_checked") and not spec.get("attempt"):  # counts that came from a run without the recount
                E2, _ = _truth.exact_counts(bbox, w, h, xs[sub], ys[sub], cap + 1, R, 2 * F, shifts=[], threads=threads)
                assert np.array_equal(exact[R][0][sub], E2), (spec["name"], R, "the guard does not suffice", exact[R][0][sub], E2)
                rec["guard_checked"] = {"samples": len(sub), "frac_bits": int(2 * F), "seconds": round(time.time() - t1, 1)}
                log("  %s R=%d: %d samples recounted at %d bits, equal, %.1f s" % (spec["name"], R, len(sub), 2 * F, time.time() - t1))
            continue
        E, st = _truth.exact_counts(bbox, w, h, xs, ys, cap + 1, R, F, shifts=ladder, threads=threads)
        guard = None
        if not spec.get("attempt"):
            t2 = time.time()
            E2, _ = _truth.exact_counts(bbox, w, h, xs[sub], ys[sub], cap + 1, R, 2 * F, shifts=[], threads=threads)
            assert np.array_equal(E[sub], E2), (spec["name"], R, "the guard does not suffice", E[sub], E2)
            guard = {"samples": len(sub), "frac_bits": int(2 * F), "seconds": round(time.time() - t2, 1)}
        bits = (st.astype(np.int64) << np.arange(len(ladder))).sum(1)
        rec = {"counts": E.astype(np.int64).tolist(), "stable_bits": bits.tolist(), "capped": int((E == 0).sum()),
               "stable_share": {str(lv): round(float(st[:, j].mean()), 4) for j, lv in enumerate(ladder)},
               "seconds": round(time.time() - t1, 1)}
        if guard:
            rec["guard_checked"] = guard
        entry["R%d" % R] = rec
        exact[R] = (E.astype(np.int64), st)
        log("  %s R=%d: %d samples, %d capped, %.1f s" % (spec["name"], R, len(xs), rec["capped"], rec["seconds"]))
    levels = {}
    for key, render in _truth.pinned_paths(v, cap, spec["pinned"]).items():
        t1 = time.time()
        R = 4 if "direct" in key else 256
        E, st = exact[R]
        got = _truth.sample_rows(render, w, xs, ys, workers=min(8, threads))
        level, per = _truth.choose_level(ladder, E, st, got, _truth.expect_minus_one(E, cap))
        # the floors count every sample stable at the level, capped ones included: the set the tests compare (_truth.misses)
        n_st = int(st[:, ladder.index(level)].sum()) if level is not None else 0
        levels[key] = {"level": level, "stable": n_st, "share": round(n_st / len(xs), 4),
                       "carries": _truth.meets_floors(n_st, len(xs)),
                       "misses_of_stable_by_level": per, "oracle_seconds": round(time.time() - t1, 1)}
        log("  %s %s: level %s  %s  %.1f s" % (spec["name"], key, level, per, time.time() - t1))
    entry["levels"] = levels
    if spec.get("scaled") and levels["m24_po"]["carries"]:
        entry["scaled"] = scaled_records(spec["name"], entry, v)
    if spec.get("hdr2x32"):
        rec = hdr2x32_escaping_orbit_record(spec["name"], entry, v)
        if rec:
            entry.setdefault("characterised", {})["hdr2x32_full"] = rec
    if spec.get("scaled"):
        rec = plain_2x32_at_record(v)
        if rec:
            entry.setdefault("excluded", {})["plain_2x32_full"] = rec
    if spec.get("attempt"):
        entry["attempt"] = True
    entry["generator_seconds"] = reuse["generator_seconds"] if reuse is not None else round(time.time() - t0, 1)
    return entry


def scaled_records(name, entry, v):
    """The scaled kernels' recorded characterisation (tests/_truth.scaled_offsets), from the restatement."""
    import _truth
    case = _truth.Case(name, entry)
    level = entry["levels"]["m24_po"]["level"]
    return {which: {"level": level, "offsets": _truth.scaled_offsets(case, v, which, level)} for which in ("hdr32", "f64")}


def hdr2x32_escaping_orbit_record(name, entry, v):
    """Where the reference orbit itself escapes (no period, fewer entries than the cap), its LA table reaches up to the orbit's
    last entry, |z|^2 > 256, while the HDRFloat<CudaDblflt> kernel's perturbation loop bails at |z|^2 >= 4 and its LA stage has
    no bailout test at all (LAKernel.cuh): an LA step carries a pixel past its escape at 4 and the count lands beyond it.  LAv2
    Full is then not an exact-count path; its offsets are recorded from the restatement."""
    import _oracle
    import _truth
    from fractalshark_amd import inputs
    o = inputs.Orbit(v, is64=True)
    if not (o.period == 0 and o.count < entry["cap"]):
        return None
    case = _truth.Case(name, entry)
    lv = entry["levels"]["m53_lav2_gpustage"]  # (on these orbits the pinned BLA function chooses no level: DESIGN.md 2.2)
    if not lv["carries"]:
        return None
    level = lv["level"]
    o2, la2 = inputs.Orbit2x32(o), inputs.LATable2x32(inputs.LATable(o, use_small_exponents=True))
    out = _oracle.gpu_lav2_2x32(v, o2, la2, mode=0, n_iterations=case.cap)
    want = _truth.expect_minus_one(case.counts(4), case.cap)
    return {"level": level, "orbit_entries": int(o.count), "offsets": _truth.offsets(case, case.sample(out), want, 4, level)}


def plain_2x32_at_record(v):
    """CudaDblflt's operator<= is `!(b > a)` (CudaDblflt.h:218-222), so ATInfo::isValid accepts the pixels OUTSIDE the AT radius
    in the plain 2x32 LAv2 kernel (tests/test_plain_oracle.py::test_2x32_at_validity_uses_the_reference_operator_as_written).
    Where that makes the kernel run AT on most pixels while the double kernel runs it on next to none, its Full mode is not an
    exact-count path and is left out of the comparison on that case; the two AT step counts are recorded as the reason."""
    import _oracle
    from fractalshark_amd import inputs
    _, s64 = _oracle.gpu_lav2_plain(v, inputs.PlainInputs(v, "f64"), mode=2, stats=True)
    _, s2 = _oracle.gpu_lav2_plain(v, inputs.PlainInputs(v, "2x32"), mode=0, stats=True)
    if not (s2["at_iterations"] >= v.width * v.height // 2 and s64["at_iterations"] <= 4):
        return None
    return {"at_iterations_2x32": int(s2["at_iterations"]), "at_iterations_f64": int(s64["at_iterations"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 2))
    ap.add_argument("--out", default=OUT, help="write here instead (a long case run on its own; merge with --merge)")
    ap.add_argument("--levels-only", action="store_true", help="keep the stored counts; choose the levels again")
    ap.add_argument("--merge", default="", help="copy the cases of this file into the fixture and stop")
    args = ap.parse_args()
    import _oracle
    import _truth
    _oracle.lib()
    out = args.out
    try:
        table = json.load(open(out))
    except (OSError, ValueError):
        table = {}
    if args.merge:
        table.setdefault("cases", {}).update(json.load(open(args.merge))["cases"])
        with open(out, "w") as f:
            json.dump(table, f, separators=(",", ":"))
        return
    table["_comment"] = (
        "Exact escape counts of sampled pixels (tests/golden/make_exact_counts.py; GMP integer iteration, no floating point, no "
        "GPU).  Per case: samples = rows x columns, row-major.  R<r>.counts = first n with |z_n|^2 > r (z_0 = 0, z_1 = c), 0 = "
        "none within cap + 1 (strict bailout; strictness is tested on exact boundary samples, tests/_truth.py); stable_bits bit j = the count is unchanged at c +- width/2^ladder[j] and c +- i width/2^ladder[j]; "
        "levels.<pinned oracle path>.level = the finest ladder level at which that path equals the expected value on every "
        "stable, uncapped sample; stable / share / carries = the samples stable at it (capped ones included) against the floors of "
        "100 samples and 20 %.")
    table.setdefault("cases", {})
    only = [x for x in args.only.split(",") if x]
    for spec in cases():
        if only and spec["name"] not in only:
            continue
        print("case", spec["name"], flush=True)
        table["cases"][spec["name"]] = build_case(spec, threads=args.threads, log=lambda s: print(s, flush=True),
                                                  reuse=table["cases"].get(spec["name"]) if args.levels_only else None)
        with open(out + ".tmp", "w") as f:
            json.dump(table, f, separators=(",", ":"))
        os.replace(out + ".tmp", out)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
