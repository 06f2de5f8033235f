"""Writes tests/golden/quiet_orbit_counts.json: per orbit of tests/_quiet_orbits.py the entries (its two spare ones included) and how many
of them have an own bound, a block bound and NDZ bounds, as the plain model (tests/_quiet_model.py) makes them.
tests/test_quiet_model_cpu.py holds the model to the file, tests/test_gpu_quiet_orbit.py the device's read-back.
Usage: python tests/golden/make_quiet_orbit_counts.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _quiet_model as qm  # noqa: E402
import _quiet_orbits as qo  # noqa: E402

WITHOUT_BOUNDS = {"period2_centre": "three entries (0, -1, -2^-193): the only entry within [2^-40, 5.6) is -1, whose smaller part is an exact "
                                    "zero, not within 2^-40 of the larger one"}

orbits = {}
for name in qo.ALL:
    t = qm.Tables(qm.prepared(qo.orbit(name).entries()))
    orbits[name] = dict(entries=t.n, **t.counts())
with open(os.path.join(HERE, "quiet_orbit_counts.json"), "w") as f:
    json.dump({"orbits": orbits, "without_bounds": WITHOUT_BOUNDS}, f, indent=1, sort_keys=True)
    f.write("\n")
