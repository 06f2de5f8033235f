"""The device half of RenderCurrent on synthetic frames, against the exact model of tests/_current.py (itself held to the
reference's CPU colouring and to plain loops by tests/test_current_model_cpu.py):

  k_antialias            both IterTypes, antialiasing 1 .. 4, the generic remainder (palettes of 1, 7, 255 and 2^24 entries, every
                         uint64 frame) and the device fast_mod at the edges of its contract (256, 257, 1792, 65536, 2^24 - 1 entries,
                         samples up to 2^32 - 1, about 65 000 per divisor), aux depths up to 31 / 63, iteration limits inside the
                         antialiasing groups, a ragged 70 x 9 colour frame, a palette that saturates the accumulators
  k_reduce               both IterTypes on frames whose padding is poisoned, at the shapes that reach the four-rows trip, the tail
                         trip, a partly valid group of four and idle waves of fsk_reduce's grid; sums that wrap at 2^64
  fs_copy_bands_to_host  the whole buffer, one block, the 2-D copy and the cut tail, into a host frame full of a sentinel
  fs_colorize_frame      a frame and a colour buffer that are not the renderer's own

The frames live in torch device tensors, and torch has to bring the GPU up before libfsmi355.so touches it: all cases run in one
fresh child process (tests/current/torch_current.py), which reports per case; every test here looks its case up."""
import json
import os
import subprocess
import sys

import pytest

import _current

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "current", "torch_current.py")


@pytest.fixture(scope="module")
def torch_child(native_libs):
    p = subprocess.run([sys.executable, CHILD], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-20000:])
    assert p.returncode == 0, p.stdout[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULTS ")][-1]
    return json.loads(line[len("RESULTS "):])


@pytest.mark.parametrize("case", _current.case_keys())
def test_case(torch_child, case):
    assert torch_child[case] == "ok"
