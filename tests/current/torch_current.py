"""Child process of tests/test_gpu_current.py: the device half of RenderCurrent -- k_antialias, k_reduce, fs_copy_bands_to_host
and fs_colorize_frame -- on synthetic frames that live in torch device tensors (SetExternalIterBuffer, and the device_iters /
device_colors arguments), against the model of tests/_current.py, every comparison exact.  torch brings the GPU up first, then
the library.  Prints one line `RESULTS {case: "ok" | traceback}`; exit status 0 when every case ran (passed or not: the parent
asserts per case)."""
import itertools
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

import _current  # noqa: E402
from fractalshark_amd import GPURenderer, _capi  # noqa: E402

# numpy may hand a new palette the address of the last one: the generation alone then tells the library to upload it
GENERATION = itertools.count(1)
SENTINEL = 0xA5


def device_tensor(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize])).to("cuda:0")
    torch.cuda.synchronize()
    return t


def host_copy(t, dtype):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def init(r, w, h, aa, pal, aux, dtype):
    n = 0 if pal is None else len(pal)
    assert r.InitializeMemory(w, h, aa, pal, n, aux, next(GENERATION), False, iter_bytes=np.dtype(dtype).itemsize) == 0


def read_frame(r):
    out = r.new_iter_buffer()
    assert r.RenderCurrent(0, out) == 0 and r.SyncComputeStream() == 0
    return out


def new_colors(r, fill=SENTINEL):
    n = int(r._lib.fs_color_buffer_elements(r._h))
    out = np.empty((n, 4), np.uint16)
    out.view(np.uint8)[...] = fill
    return out


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "%d differ, first at %s: got %s, want %s" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]) if len(bad) else ""


# ---- 3a colour
def color(r, key, p):
    frame, w, h, pal = _current.color_case_inputs(key, p)
    want = _current.colors(frame, w, h, p["aa"], pal, p["aux"], p["n_iterations"])
    t = device_tensor(frame)
    init(r, w, h, p["aa"], pal, p["aux"], frame.dtype)
    assert r.SetExternalIterBuffer(t.data_ptr(), frame.nbytes) == 0
    try:
        got, iters = new_colors(r), r.new_iter_buffer()
        assert got.shape == want.shape and iters.shape == frame.shape
        assert r.RenderCurrent(p["n_iterations"], iters, got, None, progressive=p["progressive"]) == 0
        assert (r.SyncDisplayStream() if p["progressive"] else r.SyncComputeStream()) == 0
        assert np.array_equal(got, want), first_difference(got, want)  # the zero tail beyond color_w * color_h included
        assert np.array_equal(iters, frame) and np.array_equal(host_copy(t, frame.dtype), frame)
    finally:
        assert r.SetExternalIterBuffer(None, 0) == 0


def color_no_palette(_r):
    """No palette was ever uploaded: the colour buffer comes back as InitializeMemory cleared it."""
    r = GPURenderer(0)
    try:
        frame = _current.color_frame(70, 9, np.uint32, 1792, 0, 1)
        t = device_tensor(frame)
        init(r, 70, 9, 1, None, 0, np.uint32)
        assert r.SetExternalIterBuffer(t.data_ptr(), frame.nbytes) == 0
        got = new_colors(r)
        assert r.RenderCurrent(_current.U32_CAP, None, got) == 0 and r.SyncComputeStream() == 0
        assert not got.any()
    finally:
        r.close()


def color_banded(r):
    """A renderer that holds bands of the frame colours nothing: the host colour buffer keeps its content."""
    pal = _current.injective_palette(1792)
    init(r, 70, 37, 1, pal, 0, np.uint32)
    assert r.SetRowBands(8, 8, 24) == 0
    try:
        local = _current.color_frame(70, 13, np.uint32, 1792, 0, 2)
        t = device_tensor(local)
        assert r.SetExternalIterBuffer(t.data_ptr(), local.nbytes) == 0
        got, iters = new_colors(r), r.new_iter_buffer()
        assert r.RenderCurrent(_current.U32_CAP, iters, got) == 0 and r.SyncComputeStream() == 0
        assert (got.view(np.uint8) == SENTINEL).all() and np.array_equal(iters, local)
    finally:
        assert r.SetExternalIterBuffer(None, 0) == 0 and r.SetRowBands(0, 0, 0) == 0


# ---- 3b reduction
def reduce_once(r, progressive=False):
    red = _capi.Reduction()
    assert r.RenderCurrent(0, None, None, red, progressive=progressive) == 0
    assert (r.SyncDisplayStream() if progressive else r.SyncComputeStream()) == 0
    return int(red.Min), int(red.Max), int(red.Sum)


def reduction(r, dtype, w, rows):
    init(r, w, rows, 1, None, 0, dtype)
    frames = _current.reduction_frames(w, rows, dtype, 1000 * w + rows)
    wrapped = 0
    try:
        for name, frame in frames:
            t = device_tensor(frame)
            assert r.SetExternalIterBuffer(t.data_ptr(), frame.nbytes) == 0
            want = _current.reduction(frame, w, rows, dtype)
            got = reduce_once(r)
            assert got == want, (name, got, want)
            if name == "all_equal":
                assert got[0] == got[1]
            if np.dtype(dtype).itemsize == 8:
                wrapped += int(frame[:rows, :w].astype(object).sum() >= 2 ** 64)
    finally:
        assert r.SetExternalIterBuffer(None, 0) == 0
    if np.dtype(dtype).itemsize == 8 and w * rows > 2:
        assert wrapped == len(frames)  # the true sum passes 2^64: the expected value is the wrapped one


def reduction_banded(r, dtype):
    """h = 37 under SetRowBands(8, 8, 24): the 13 local rows and nothing of the three padding rows behind them."""
    init(r, 18, 37, 1, None, 0, dtype)
    assert r.SetRowBands(8, 8, 24) == 0
    try:
        assert r.local_rows == 16
        for name, frame in _current.reduction_frames(18, 13, dtype, 5):
            t = device_tensor(frame)
            assert r.SetExternalIterBuffer(t.data_ptr(), frame.nbytes) == 0
            assert reduce_once(r) == _current.reduction(frame, 18, 13, dtype), name
    finally:
        assert r.SetExternalIterBuffer(None, 0) == 0 and r.SetRowBands(0, 0, 0) == 0


def reduction_progressive(r, dtype):
    init(r, 1030, 5, 1, None, 0, dtype)
    try:
        for name, frame in _current.reduction_frames(1030, 5, dtype, 6)[:2]:
            t = device_tensor(frame)
            assert r.SetExternalIterBuffer(t.data_ptr(), frame.nbytes) == 0
            want = _current.reduction(frame, 1030, 5, dtype)
            assert reduce_once(r, progressive=True) == want and reduce_once(r) == want, name
    finally:
        assert r.SetExternalIterBuffer(None, 0) == 0


# ---- 3c fs_copy_bands_to_host
def copy_bands(r, dtype, cfg, source):
    H, first, rows, stride = cfg
    w, dtype = _current.BAND_W, np.dtype(dtype)
    rng = np.random.default_rng(H * 100 + first + dtype.itemsize)
    top = _current.ALL_ONES[dtype]
    whole = _current.poisoned(rng.integers(1, top - 1, (H, w), dtype=np.uint64, endpoint=True).astype(dtype), dtype)
    local, image = _current.bands(whole[:H], H, first, rows, stride, SENTINEL)
    n_local = len(local)
    # the local buffer with its poisoned padding rows, and a frame's worth of poisoned rows behind it
    buf = _current.poisoned(local[:, :w], dtype, extra_rows=_current.padded_rows(H))
    buf[:n_local] = local
    init(r, w, H, 1, None, 0, dtype)
    assert r.SetRowBands(first, rows, stride) == 0
    try:
        lrp = _current.padded_rows(n_local)
        assert r.local_rows == lrp and r.rounded_width == whole.shape[1]
        t = device_tensor(buf)
        other = np.full_like(buf, 3)
        t_own = t if source == "own" else device_tensor(other)
        assert r.SetExternalIterBuffer(t_own.data_ptr(), buf.nbytes) == 0
        host = np.empty_like(whole)
        host.view(np.uint8)[...] = SENTINEL
        want = host.copy()
        if rows == 0:
            want[:lrp] = buf[:lrp]  # no banding: the whole padded buffer
        else:
            want[:H] = image
        assert r.CopyBandsToHost(host.ctypes.data, None if source == "own" else t.data_ptr()) == 0
        assert r.SyncComputeStream() == 0
        assert np.array_equal(host, want), first_difference(host, want)
        if source != "own":  # the renderer's own buffer keeps its content
            assert np.array_equal(read_frame(r), other[:lrp]) and np.array_equal(host_copy(t_own, dtype), other)
        assert np.array_equal(host_copy(t, dtype), buf)
    finally:
        assert r.SetExternalIterBuffer(None, 0) == 0 and r.SetRowBands(0, 0, 0) == 0


# ---- 3d fs_colorize_frame
def colorize(r, dtype, aa, dst):
    dtype = np.dtype(dtype)
    cw, ch = _current.COLOR_W, _current.COLOR_H
    w, h = cw * aa, ch * aa
    cap = _current.U32_CAP if dtype.itemsize == 4 else _current.U64_CAP
    pal = _current.injective_palette(1792 if dtype.itemsize == 4 else 7)
    own = _current.color_frame(w, h, dtype, len(pal), 0, 40 + aa)
    frame = _current.color_frame(w, h, dtype, len(pal), 0, 50 + aa)
    t_own, t_frame = device_tensor(own), device_tensor(frame)
    init(r, w, h, aa, pal, 0, dtype)
    assert r.SetExternalIterBuffer(t_own.data_ptr(), own.nbytes) == 0
    try:
        mine = new_colors(r)
        assert r.RenderCurrent(cap, None, mine) == 0 and r.SyncComputeStream() == 0
        want_own = _current.colors(own, w, h, aa, pal, 0, cap)
        assert np.array_equal(mine, want_own)
        want = _current.colors(frame, w, h, aa, pal, 0, cap)
        assert not np.array_equal(want, want_own)
        got, kept = new_colors(r), new_colors(r, 0)
        if dst == "tensor":
            t_colors = device_tensor(new_colors(r))
            want[cw * ch:].view(np.uint8)[...] = SENTINEL  # the kernel writes color_w * color_h pixels, the copy takes all
            assert r._lib.fs_colorize_frame(r._h, t_frame.data_ptr(), cap, t_colors.data_ptr(), got.ctypes.data,
                                            r.compute_stream) == 0
            assert r.SyncComputeStream() == 0
            assert np.array_equal(got, want), first_difference(got, want)
            assert np.array_equal(host_copy(t_colors, np.uint16).reshape(-1, 4), want)
            assert r._lib.fs_read_color_buffer(r._h, kept.ctypes.data) == 0
            assert np.array_equal(kept, want_own)  # the renderer's own colour buffer is as RenderCurrent left it
        else:
            assert r._lib.fs_colorize_frame(r._h, t_frame.data_ptr(), cap, None, got.ctypes.data, r.compute_stream) == 0
            assert r.SyncComputeStream() == 0
            assert np.array_equal(got, want), first_difference(got, want)
            assert r._lib.fs_read_color_buffer(r._h, kept.ctypes.data) == 0
            assert np.array_equal(kept, want)
        assert np.array_equal(read_frame(r), own) and np.array_equal(host_copy(t_own, dtype), own)
        assert np.array_equal(host_copy(t_frame, dtype), frame)
    finally:
        assert r.SetExternalIterBuffer(None, 0) == 0


def colorize_no_palette(_r):
    """Without a palette the call returns 0 and writes nothing: not device_colors, not the host buffer, not the renderer's own."""
    r = GPURenderer(0)
    try:
        frame = _current.color_frame(140, 18, np.uint32, 1792, 0, 9)
        t_frame = device_tensor(frame)
        init(r, 140, 18, 2, None, 0, np.uint32)
        got, kept = new_colors(r), new_colors(r)
        t_colors = device_tensor(got)
        for dev in (t_colors.data_ptr(), None):
            assert r._lib.fs_colorize_frame(r._h, t_frame.data_ptr(), _current.U32_CAP, dev, got.ctypes.data,
                                            r.compute_stream) == 0
            assert r.SyncComputeStream() == 0
        assert (got.view(np.uint8) == SENTINEL).all()
        assert (host_copy(t_colors, np.uint8) == SENTINEL).all()
        assert r._lib.fs_read_color_buffer(r._h, kept.ctypes.data) == 0 and not kept.any()
    finally:
        r.close()


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

    for key, p in _current.color_cases().items():
        run("color-" + key, color, key, p)
    run("color-no_palette", color_no_palette)
    run("color-banded", color_banded)
    for dtype in ("uint32", "uint64"):
        for w, rows in _current.REDUCTION_SHAPES[dtype]:
            run("reduce-%s-%dx%d" % (dtype, w, rows), reduction, dtype, w, rows)
        run("reduce-%s-banded" % dtype, reduction_banded, dtype)
        run("reduce-%s-progressive" % dtype, reduction_progressive, dtype)
        for cfg in _current.BAND_CONFIGS:
            for source in ("own", "device_iters"):
                run("bands-%s-%d_%d_%d_%d-%s" % ((dtype,) + cfg + (source,)), copy_bands, dtype, cfg, source)
        for aa in (2, 4):
            for dst in ("tensor", "null"):
                run("colorize-%s-aa%d-%s" % (dtype, aa, dst), colorize, dtype, aa, dst)
    run("colorize-no_palette", colorize_no_palette)
    r.close()
    assert sorted(results) == sorted(_current.case_keys())
    print("RESULTS " + json.dumps(results))


if __name__ == "__main__":
    main()
