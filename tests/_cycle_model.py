"""The exact renderer's cycle check restated on Python integers -- the model the CPU and GPU tests of the check compare with
(tests/test_exact_cycle_cpu.py, tests/test_gpu_exact_cycle.py).  Written from the rule, not from csrc/exact_cycle_math.hpp:

  n is the index of the z a sample holds, z_1 = c.  A step tests z_n for escape (|z_n|^2 > R, >= when inclusive: value n - 1), then
  for the cap (n == cap + 1: value cap, unproved), and otherwise replaces z_n by z_{n+1} and increments n.  The sample carries a
  checkpoint, z_1 at first.  After the increment: the state equals the checkpoint -> proved (value cap); otherwise, n a power of two
  -> the checkpoint becomes the state.

Besides outcome, value and steps the model counts how often the low 1, 4 and 64 bits of the 64-bit number (low limb of y : low limb
of x) equal the checkpoint's after an increment: the steps on which a kernel with such a fingerprint must read its checkpoint back.
"""
import json
import os
import zlib

import numpy as np

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_cycle_model.json")

ESCAPED, CAPPED, PROVED = 0, 1, 2
M32 = 0xFFFFFFFF


def sample(cx, cy, F, R, inclusive, cap):
    """(outcome, value, steps, (hits1, hits4, hits64)) of c = (cx + i cy) / 2^F."""
    bail = R << (2 * F)
    x, y, tx, ty, n, steps = cx, cy, cx, cy, 1, 0
    h1 = h4 = h64 = 0
    while True:
        steps += 1
        xx, yy = x * x, y * y
        s = xx + yy
        if s > bail or (inclusive and s == bail):
            return ESCAPED, n - 1, steps, (h1, h4, h64)
        if n == cap + 1:
            return CAPPED, cap, steps, (h1, h4, h64)
        x, y = ((xx - yy) >> F) + cx, ((2 * x * y) >> F) + cy
        n += 1
        dx = x ^ tx
        if not dx & 1:
            h1 += 1
            if not dx & 15:
                h4 += 1
                dy = y ^ ty
                if not dx & M32 and not dy & M32:
                    h64 += 1
                    if dx == 0 and dy == 0:
                        return PROVED, cap, steps, (h1, h4, h64)
        if n & (n - 1) == 0:
            tx, ty = x, y


def from_limbs(a):
    """uint32[limbs, n] (two's complement, limb-major) -> n Python integers."""
    a = np.asarray(a, np.uint32)
    L = a.shape[0]
    out = []
    for i in range(a.shape[1]):
        v = sum(int(a[l, i]) << (32 * l) for l in range(L))
        out.append(v - (1 << (32 * L)) if v >> (32 * L - 1) else v)
    return out


class Runs:
    """The model over a list of samples (cxs[i], cys[i]): outcome, value, steps as arrays, hits = int64[n, 3]."""

    def __init__(self, cxs, cys, F, R, inclusive, cap, only=None):
        """only: the model is run on these samples alone (the others read as escaped at once)."""
        idle = (ESCAPED, 0, 1, (0, 0, 0))
        res = [sample(a, b, F, R, inclusive, cap) if only is None or i in only else idle for i, (a, b) in enumerate(zip(cxs, cys))]
        self._set([r[0] for r in res], [r[2] for r in res], cap)
        self.hits = np.array([r[3] for r in res], np.int64).reshape(len(res), 3)
        self.hit_totals = tuple(int(v) for v in self.hits.sum(axis=0))

    def _set(self, outcome, steps, cap):
        self.outcome, self.steps = np.array(outcome, np.int64), np.array(steps, np.int64)
        self.value = np.where(self.outcome == ESCAPED, self.steps - 1, cap)  # an escape at E = its steps leaves E - 1
        self.proved = self.outcome == PROVED
        # what the same samples cost without the check: E steps to an escape at E, cap + 1 otherwise
        self.steps_off = np.where(self.outcome == ESCAPED, self.value + 1, cap + 1)

    def kinds(self):
        """(escaping, proved, capped and unproved)"""
        return tuple(int((self.outcome == k).sum()) for k in (ESCAPED, PROVED, CAPPED))


def frame(cx_axis, cy_axis, F, R, inclusive, cap, only=None):
    """Runs over the row-major W x H frame of the axes (Python integers per column / row)."""
    w = len(cx_axis)
    cxs = list(cx_axis) * len(cy_axis)
    cys = [v for v in cy_axis for _ in range(w)]
    return Runs(cxs, cys, F, R, inclusive, cap, only)


# ---- recorded results.  The model of a 64 x 48 frame at 758 fractional bits is four million steps on Python integers of 24 limbs:
# a quarter of a minute.  tests/golden/make_exact_cycle_model.py runs this module on the frames the GPU tests use and records what it
# says (tests/golden/exact_cycle_model.json); the CPU test runs the model again on a part of every record.
def axes_crc(cx, cy):
    """What a record is tied to: the axes (uint32[limbs, W], uint32[limbs, H]) the model was run on."""
    return zlib.crc32(np.ascontiguousarray(cy, np.uint32).tobytes(), zlib.crc32(np.ascontiguousarray(cx, np.uint32).tobytes()))


def record_key(w, h, F, R, inclusive, cap):
    return "%dx%d_F%d_R%d_%s_cap%d" % (w, h, F, R, "inclusive" if inclusive else "strict", cap)


def to_record(runs, crc):
    return {"axes_crc": crc, "outcome": "".join(str(int(o)) for o in runs.outcome), "steps": [int(s) for s in runs.steps],
            "hit_totals": list(runs.hit_totals)}


_records = None


def recorded(key, crc, cap):
    """The recorded Runs for the key (hits: totals only), None when there is no record; the record must be of the same axes."""
    global _records
    if _records is None:
        with open(RECORD) as f:
            _records = json.load(f)["frames"]
    rec = _records.get(key)
    if rec is None:
        return None
    assert rec["axes_crc"] == crc, "the recorded model was made for other axes: run tests/golden/make_exact_cycle_model.py"
    runs = Runs.__new__(Runs)
    runs._set([int(ch) for ch in rec["outcome"]], rec["steps"], cap)
    runs.hits, runs.hit_totals = None, tuple(rec["hit_totals"])
    return runs
