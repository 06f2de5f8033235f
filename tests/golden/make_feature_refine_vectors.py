#!/usr/bin/env python3
"""Writes tests/golden/feature_refine_vectors.json: tests/_point_model.py's refinement of the 86 found points of
tests/golden/feature_vectors.json (View 5) at 704 fractional bits, bailout 256, 16 rounds -- per point its status, the refined c
(integers, c 2^704, as decimal strings; null where nothing was evaluated to its end), the atom period there and the number of
evaluations.  Python integers only: a couple of minutes on one core; --jobs N spreads the points over N processes."""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _point_model as model  # noqa: E402

F, ROUNDS, BAILOUT = 704, 16, 256


def one(pt):
    c0, delta, p = model.fixture_point(pt, F)
    r = model.refine(c0, delta, p, F, ROUNDS, BAILOUT)
    return {"status": r["status"], "cx": None if r["c"] is None else str(r["c"][0]), "cy": None if r["c"] is None else str(r["c"][1]),
            "atom": r["atom"], "evaluations": r["evaluations"], "converged": r["converged"]}


def main():
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 1
    found = model.fixture()
    with ProcessPoolExecutor(jobs) as ex:
        points = list(ex.map(one, found))
    count = lambda s: sum(1 for q in points if q["status"] == s)
    print("fixed %d rounds %d stalled %d escaped %d converged %d" % (count("fixed"), count("rounds"), count("stalled"), count("escaped"),
                                                                   sum(1 for q in points if q["converged"])))
    with open(model.RECORD, "w") as f:
        json.dump({"frac_bits": F, "rounds": ROUNDS, "bailout": BAILOUT, "points": points}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
