#!/usr/bin/env python3
"""Writes tests/golden/exact_cycle_model.json: what the Python-integer model of the exact renderer's cycle check
(tests/_cycle_model.py) says about the frames tests/test_gpu_exact_cycle.py renders -- per sample the outcome (0 escaped, 1 capped
and unproved, 2 proved) and the steps taken, per frame how often the low 1, 4 and 64 bits of the state matched the checkpoint.
The frame at 758 fractional bits takes the model a quarter of a minute; the whole file about half a minute.  CPU only (the axes come
from libfsinputs).  tests/test_exact_cycle_cpu.py runs the model again on a part of every record.

    python tests/golden/make_exact_cycle_model.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _cycle_model as model  # noqa: E402
from fractalshark_amd import exact, inputs  # noqa: E402

BBOX, W, H, CAP = ("-2.2", "-1.2", "1.0", "1.2"), 64, 48, 20000
FRAMES = [(54, 4, False), (246, 4, False), (758, 4, False), (246, 256, False), (246, 4, True)]  # (frac_bits, R, inclusive)

if __name__ == "__main__":
    v = inputs.View(*BBOX, W, H)
    frames = {}
    for F, R, inclusive in FRAMES:
        cx, cy = exact.axes(v, F)
        runs = model.frame(model.from_limbs(cx), model.from_limbs(cy), F, R, inclusive, CAP)
        key = model.record_key(W, H, F, R, inclusive, CAP)
        frames[key] = model.to_record(runs, model.axes_crc(cx, cy))
        print(key, "escaped / proved / capped", runs.kinds(), "steps", int(runs.steps.sum()), "without the check", int(runs.steps_off.sum()),
              "matches of 1 / 4 / 64 bits", runs.hit_totals, flush=True)
    with open(model.RECORD, "w") as f:
        json.dump({"bbox": list(BBOX), "width": W, "height": H, "cap": CAP, "frames": frames}, f, separators=(",", ":"))
        f.write("\n")
