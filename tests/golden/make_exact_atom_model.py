#!/usr/bin/env python3
"""Writes tests/golden/exact_atom_model.json: what the Python-integer model of the exact renderer's period planes
(tests/_atom_model.py) says about the frames tests/test_gpu_exact_atom.py renders -- per sample the value, the atom period and the
cycle length (0: not proved).  The model runs the definition: every sample to its escape or to the cap, WITHOUT the cycle check --
twelve million steps per 64 x 48 frame, on integers of up to 24 limbs; the whole file takes a few minutes on --jobs processes.  CPU
only (the axes come from libfsinputs).  tests/test_exact_atom_cpu.py runs the model again on a part of every record.

    python tests/golden/make_exact_atom_model.py [--jobs 8]
"""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _atom_model as model  # noqa: E402
import _cycle_model as cycle  # noqa: E402
import _truth  # noqa: E402
from fractalshark_amd import exact, inputs  # noqa: E402

BBOX, W, H, CAP = ("-2.2", "-1.2", "1.0", "1.2"), 64, 48, 20000
FRAMES = [(54, 4, False), (246, 4, False), (758, 4, False), (246, 256, False), (246, 4, True)]  # (frac_bits, R, inclusive)


def _row(args):
    ax, cyv, F, R, inclusive, cap = args
    return [model.sample(a, cyv, F, R, inclusive, cap, check=False) for a in ax]


def _frame(pool, view, w, h, F, R, inclusive, cap):
    cx, cy = exact.axes(view, F)
    ax, ay = cycle.from_limbs(cx), cycle.from_limbs(cy)
    rows = list(pool.map(_row, [(ax, v, F, R, inclusive, cap) for v in ay]))
    planes = model.Planes.__new__(model.Planes)
    flat = [s for row in rows for s in row]
    planes.value, planes.atom, planes.cyclen = ([s[k] for s in flat] for k in (0, 1, 3))
    key = model.record_key(w, h, F, R, inclusive, cap)
    print(key, "proved", sum(1 for s in flat if s[3]), "atom periods", len(set(s[1] for s in flat)), flush=True)
    return key, model.to_record(planes, cycle.axes_crc(cx, cy))


if __name__ == "__main__":
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 8
    frames = {}
    with ProcessPoolExecutor(jobs) as pool:
        v = inputs.View(*BBOX, W, H)
        for F, R, inclusive in FRAMES:
            key, rec = _frame(pool, v, W, H, F, R, inclusive, CAP)
            frames[key] = rec
        c = _truth.Case("view0_70x37")
        key, rec = _frame(pool, c.view(inputs), c.w, c.h, c.raw["frac_bits"], 4, False, c.cap)
        frames[key] = rec
    with open(model.RECORD, "w") as f:
        json.dump({"bbox": list(BBOX), "width": W, "height": H, "cap": CAP, "frames": frames}, f, separators=(",", ":"))
        f.write("\n")
