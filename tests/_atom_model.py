"""The exact renderer's period planes restated on Python integers -- the model the CPU and GPU tests of the planes compare with
(tests/test_exact_atom_cpu.py, tests/test_gpu_exact_atom.py).  Written from the definitions, not from csrc/exact_atom_math.hpp:

  n is the index of the z a sample holds, z_1 = c.  N_n = x_n^2 + y_n^2, untruncated.  E is the first n at which z_n escapes
  (N_n > R 2^2F, >= when inclusive); the value is v = min(E - 1, cap).  The tracked states are z_1 .. z_v.  The atom period A is the
  n in 1 .. v with the smallest N_n, the earliest such n; 0 when v = 0.
  A sample the cycle check proves at index n equals its checkpoint, taken at t: the cycle length is n - t, 0 when it is not proved.
  Which samples are proved and at which n is the word of tests/_cycle_model.py (the proof index is its steps + 1: a sample holds z_n
  after n - 1 steps); its rule takes the checkpoint at n = 1 and then at every power of two AFTER the comparison at that n, so the
  checkpoint a comparison at n sees is that of the largest power of two below n.

`//` and `>>` on Python integers floor.  Besides the values the model counts how often a kernel whose register-side key of the
minimum is the narrowest the header allows -- the index of the highest 32-bit limb of N that is not zero, nothing else -- must read
the whole minimum back: at every tracked n > 1 whose key is neither less nor greater than the minimum's.
"""
import json
import os

import numpy as np

import _cycle_model as cycle

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_atom_model.json")


def checkpoint_index(n):
    """The index at which the checkpoint a comparison at n >= 2 sees was taken: the largest power of two below n."""
    return 1 << ((n - 1).bit_length() - 1)


def _top_limb(N):
    return (N.bit_length() - 1) // 32 if N else 0


def sample(cx, cy, F, R, inclusive, cap, check=False):
    """(v, A, proof index, cycle length, read-backs) of c = (cx + i cy) / 2^F.  The proof index and the cycle length are 0 for a
    sample the cycle check does not prove within the cap.  check: the sample stops at its proof, as the kernels with the cycle check
    do; v and A are defined without it and must come out the same (the tests compare the two)."""
    outcome, value, steps, _ = cycle.sample(cx, cy, F, R, inclusive, cap)
    proof_n = steps + 1 if outcome == cycle.PROVED else 0
    lam = proof_n - checkpoint_index(proof_n) if proof_n else 0
    stop = proof_n if check else 0
    bail = R << (2 * F)
    x, y, n = cx, cy, 1
    A, best, best_top, readbacks = 0, None, 0, 0
    while True:
        xx, yy = x * x, y * y
        N = xx + yy
        if N > bail or (inclusive and N == bail):
            v = n - 1
            break
        if n == cap + 1:
            v = cap
            break
        if n == 1:
            A, best, best_top = 1, N, _top_limb(N)
        else:
            top = _top_limb(N)
            if top == best_top:
                readbacks += 1
            if N < best:
                A, best, best_top = n, N, top
        x, y = ((xx - yy) >> F) + cx, ((2 * x * y) >> F) + cy
        n += 1
        if n == stop:
            v = cap
            break
    assert v == value and A <= v
    return v, A, proof_n, lam, readbacks


class Planes:
    """The model over a list of samples: value, atom, proof_n, cyclen and readbacks as int64 arrays."""

    def __init__(self, cxs, cys, F, R, inclusive, cap, check=False, only=None):
        """only: the model is run on these samples alone (the others read as zeros)."""
        idle = (0, 0, 0, 0, 0)
        res = [sample(a, b, F, R, inclusive, cap, check) if only is None or i in only else idle for i, (a, b) in enumerate(zip(cxs, cys))]
        cols = np.array(res, np.int64).reshape(len(res), 5)
        self.value, self.atom, self.proof_n, self.cyclen, self.readbacks = (cols[:, k].copy() for k in range(5))


def frame(cx_axis, cy_axis, F, R, inclusive, cap, check=False, only=None):
    """Planes over the row-major W x H frame of the axes (Python integers per column / row)."""
    w = len(cx_axis)
    cxs = list(cx_axis) * len(cy_axis)
    cys = [v for v in cy_axis for _ in range(w)]
    return Planes(cxs, cys, F, R, inclusive, cap, check, only)


# ---- recorded results (the scheme of _cycle_model.py: a 64 x 48 frame at 758 fractional bits WITHOUT the cycle check is twelve
# million steps on Python integers of 24 limbs).  tests/golden/make_exact_atom_model.py runs this module on the frames the GPU tests
# use and records what it says (tests/golden/exact_atom_model.json); the CPU test runs the model again on a part of every record.
def record_key(w, h, F, R, inclusive, cap):
    return cycle.record_key(w, h, F, R, inclusive, cap)


def to_record(planes, crc):
    return {"axes_crc": crc, "value": [int(v) for v in planes.value], "atom": [int(v) for v in planes.atom],
            "cyclen": [int(v) for v in planes.cyclen]}


_records = None


def recorded(key, crc):
    """The recorded (value, atom, cyclen) int64 arrays for the key, None when there is no record; the record must be of the same axes."""
    global _records
    if _records is None:
        with open(RECORD) as f:
            _records = json.load(f)["frames"]
    rec = _records.get(key)
    if rec is None:
        return None
    assert rec["axes_crc"] == crc, "the recorded model was made for other axes: run tests/golden/make_exact_atom_model.py"
    return tuple(np.array(rec[k], np.int64) for k in ("value", "atom", "cyclen"))
