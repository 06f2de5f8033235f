"""Child process of tests/test_gpu_exact_audit.py: fs_exact_audit on a frame that lives in a torch device tensor (the device_iters
argument).  torch brings the GPU up first, then the library.  Prints one line `RESULTS {case: "ok" | traceback}`; exit status 0
when every case ran (passed or not: the parent asserts per case)."""
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

import _truth  # noqa: E402
from fractalshark_amd import GPURenderer, exact, inputs  # noqa: E402


def read_frame(r, n):
    out = r.new_iter_buffer()
    assert r.RenderCurrent(n, out) == 0 and r.SyncComputeStream() == 0
    return out


def device_iters(r):
    """A copy of the exact frame with a few sample pixels and a few other pixels altered: only the altered samples are reported,
    and the renderer's own buffer keeps its content."""
    c = _truth.Case("shallow_1e-20")
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0 and r.ClearMemory() == 0
    exact.render(r, v, bailout=256, frac_bits=F)
    own = read_frame(r, c.cap)
    levels = (17, 30)
    assert exact.audit(r, v, c.xs, c.ys, levels=levels, bailout=256, frac_bits=F).n_differ == 0
    altered = own.copy()
    picked = [5, 64, 300, 575]                       # sample indices
    for k, i in enumerate(picked):
        altered[c.ys[i], c.xs[i]] += 3 + k
    sampled = set(zip(c.xs.tolist(), c.ys.tolist()))
    others = [(x, y) for y in (1, 3, 17) for x in (1, 3, 33) if (x, y) not in sampled][:4]
    assert len(others) == 4                          # the lattice of 32 x 18 in 64 x 36 leaves pixels out
    for x, y in others:
        altered[y, x] += 1000
    t = torch.from_numpy(altered.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    rep = exact.audit(r, v, c.xs, c.ys, levels=levels, bailout=256, frac_bits=F, device_iters=t.data_ptr())
    assert rep.n_differ == 4 and [o["sample"] for o in rep.offenders] == picked
    assert [o["frame_value"] - o["exact_value"] for o in rep.offenders] == [3, 4, 5, 6]
    assert np.array_equal(rep.frame_values, altered[c.ys, c.xs].astype(np.int64))
    assert np.array_equal(rep.values, own[c.ys, c.xs].astype(np.int64))
    assert np.array_equal(t.cpu().numpy().view(np.uint32), altered)        # the tensor is only read
    assert read_frame(r, c.cap).tobytes() == own.tobytes()
    assert exact.audit(r, v, c.xs, c.ys, levels=levels, bailout=256, frac_bits=F).n_differ == 0


def main():
    assert GPURenderer.TestCudaIsWorking() != 0
    r = GPURenderer(0)
    results = {}
    try:
        device_iters(r)
        results["device_iters"] = "ok"
    except Exception:  # reported per case
        results["device_iters"] = traceback.format_exc()
        print(results["device_iters"])
    r.close()
    print("RESULTS " + json.dumps(results))


if __name__ == "__main__":
    main()
