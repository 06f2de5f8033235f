"""Child process of tests/test_gpu_autozoom.py: fs_autozoom_pick on synthetic frames that live in torch device tensors
(SetExternalIterBuffer, and the device_iters argument).  torch brings the GPU up first, then the library.  Prints one line
`RESULTS {case: "ok" | traceback}`; exit status 0 when every case ran (passed or not: the parent asserts per case)."""
import json
import os
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()  # before libfsmi355.so touches the device

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _autozoom  # noqa: E402
from fractalshark_amd import GPURenderer, autozoom  # noqa: E402

SYNTHETIC = {"lattice": (_autozoom.lattice, _autozoom.LATTICE_N), "constant": (_autozoom.constant, 100),
             "mirror": (_autozoom.mirror, 100), "last_row_tip": (_autozoom.last_row_tip, 100)}


def device_tensor(frame):
    t = torch.from_numpy(frame.view(np.int64 if frame.dtype == np.uint64 else np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def synthetic(r, name, cap_rows, dtype):
    make, n = SYNTHETIC[name]
    valid = make()
    h, w = valid.shape
    frame = _autozoom.padded(valid, dtype)
    t = device_tensor(frame)
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False, iter_bytes=frame.itemsize) == 0
    assert r.SetExternalIterBuffer(t.data_ptr(), frame.nbytes) == 0
    assert r.SetAutozoomGatherCap(cap_rows) == 0
    try:
        got = _autozoom.check_against_checker(r, frame, w, h, 1, n)
        assert np.array_equal(_autozoom.read_frame(r, n), frame)
    finally:
        assert r.SetAutozoomGatherCap(0) == 0
        assert r.SetExternalIterBuffer(None, 0) == 0
    tip = got["tip"]
    if name == "lattice":
        # 968 exact ties at score 0: with two rows of gather buffer (288 records) the band path decides, and decides the same
        assert (tip.target_x, tip.target_y, tip.score, tip.accepted, tip.rescored) == (20, 20, 0.0, 968, 968)
    elif name == "constant":
        assert got["max"].status == got["default"].status == autozoom.FLAT and tip.status == autozoom.NO_TARGET
    elif name == "mirror":
        assert (tip.target_x, tip.target_y, tip.rescored) == (30, 40, 2)  # the winner and its mirror image tie
    else:
        assert (tip.target_x, tip.target_y) == (w - 19, h - 19)


def device_iters(r):
    """A frame handed over as device_iters is analysed in place of the current buffer, which keeps its content."""
    valid = _autozoom.mirror()
    h, w = valid.shape
    frame = _autozoom.padded(valid)
    t = device_tensor(frame)
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False) == 0
    assert r.ClearMemory() == 0 and r.SyncComputeStream() == 0
    _autozoom.check_against_checker(r, frame, w, h, 1, 100, device_iters=t.data_ptr())
    assert _autozoom.gpu_pick(r, autozoom.MAX, 100).status == autozoom.FLAT  # the cleared buffer of the renderer itself
    assert not _autozoom.read_frame(r, 100).any()


def main():
    assert GPURenderer.TestCudaIsWorking() != 0
    r = GPURenderer(0)
    results = {}

    def run(key, fn, *args):
        try:
            fn(r, *args)
            results[key] = "ok"
        except Exception:  # reported per case
            results[key] = traceback.format_exc()
            print(key, results[key])

    for name in sorted(SYNTHETIC):
        for cap_rows in (0, 2):
            for dtype in (np.uint32, np.uint64):
                run("%s-%d-%s" % (name, cap_rows, np.dtype(dtype).name), synthetic, name, cap_rows, dtype)
    run("device_iters", device_iters)
    r.close()
    print("RESULTS " + json.dumps(results))


if __name__ == "__main__":
    main()
