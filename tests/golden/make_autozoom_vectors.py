"""Writes tests/golden/autozoom_vectors.json: the records of the sequential checker (tests/autozoom/autozoom_ref.cpp) for the
three heuristics on CPU-oracle frames (View 0 direct, View 5 LAv2) and on synthetic frames (tests/_autozoom.py), both IterTypes.
Floats are stored as hexadecimal text: the fixture pins every bit.  Run from the repository root:
    python tests/golden/make_autozoom_vectors.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _autozoom  # noqa: E402


def main():
    out = {}
    for name, (frame, w, h, aa, n) in sorted(_autozoom.frames().items()):
        out[name] = {"width": w, "height": h, "antialiasing": aa, "n_iterations": n}
        for hname, heur in sorted(_autozoom.HEURISTICS.items()):
            rec = _autozoom.as_dict(_autozoom.ref_pick(frame, w, h, heur, n, aa))
            assert rec == _autozoom.as_dict(_autozoom.ref_pick(frame.astype(np.uint64), w, h, heur, n, aa)), (name, hname)
            out[name][hname] = rec
    with open(_autozoom.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", _autozoom.GOLDEN)


if __name__ == "__main__":
    main()
