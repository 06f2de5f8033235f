"""CPU-only: the reference model of RenderCurrent's device half (tests/_current.py) held to two independent statements of the
same operations -- the reference's own CPU colouring through the pin library (oracle/png_pin.cpp: PngParallelSave::Run, doubles
and a PNG encoder, no line shared with the model), and plain Python loops over tiny frames -- before tests/test_gpu_current.py
holds the kernels to the model."""
import numpy as np
import pytest

import _current
import _oracle


# ---- the model against the reference's CPU colouring
def _crc_frames(aa):
    """uint32 frames for colour size 70 x 9: one with the limit 1000 and samples 998 .. 1002 inside the antialiasing groups, one
    with the limit INT32_MAX - 1 (GetMaxIterations<uint32_t>: the pin's clamp never acts below it) and samples over the whole
    type, about half of them at or above it."""
    w, h = _current.COLOR_W * aa, _current.COLOR_H * aa
    yield _current.color_frame(w, h, np.uint32, 1792, 0, 11 + aa, cap=1000, below=2000), 1000
    yield _current.color_frame(w, h, np.uint32, 1792, 0, 23 + aa), 2 ** 31 - 2


@pytest.mark.parametrize("aa", [1, 2, 3, 4])
def test_model_reproduces_the_reference_cpu_colouring(native_libs, aa):
    pal = _oracle.default_palette(8)
    cw, ch = _current.COLOR_W, _current.COLOR_H
    for frame, n_iterations in _crc_frames(aa):
        valid = frame[:ch * aa, :cw * aa]
        groups = (valid.reshape(ch, aa, cw, aa) < n_iterations).sum(axis=(1, 3))
        if aa > 1:  # coloured and uncoloured samples inside single groups
            assert ((groups > 0) & (groups < aa * aa)).sum() > cw * ch // 4
        model = _current.colors(frame, cw * aa, ch * aa, aa, pal, 0, n_iterations)
        assert model.shape == (80 * 16, 4) and not model[cw * ch:].any() and (model[:cw * ch, 3] == 65535).all()
        if _oracle.pin_lib() is not None:
            want = _oracle.png_crc64(frame, cw, ch, aa, n_iterations)
            assert _oracle.png_crc64_rgba16(model[:cw * ch].reshape(ch, cw, 4), cw, ch) == want


# ---- the model against plain loops
def _colors_loop(frame, w, h, aa, pal, aux_depth, n_iterations):
    out = []
    for oy in range(h // aa):
        for ox in range(w // aa):
            acc = [0, 0, 0]
            for iy in range(oy * aa, (oy + 1) * aa):
                for ix in range(ox * aa, (ox + 1) * aa):
                    n = int(frame[iy, ix])
                    if n < n_iterations:
                        e = pal[(n >> aux_depth) % len(pal)]
                        for k in range(3):
                            acc[k] += int(e[k])
            out.append([a // (aa * aa) for a in acc] + [65535])
    return out


@pytest.mark.parametrize("dtype,aux,n_iterations", [(np.uint32, 0, 2 ** 32 - 1), (np.uint32, 5, 1000), (np.uint64, 33, 2 ** 64 - 1),
                                                    (np.uint64, 0, 2 ** 32 + 1000)])
@pytest.mark.parametrize("aa", [1, 2, 3, 4])
def test_colors_against_a_plain_loop(aa, dtype, aux, n_iterations):
    for pal in (_current.injective_palette(257), _current.saturating_palette()):
        w = h = 2 * aa
        cap = n_iterations if n_iterations < 2 ** 40 else None
        frame = _current.color_frame(w, h, dtype, len(pal), aux, 5 + aa, cap=cap, below=2 * cap if cap else None)
        got = _current.colors(frame, w, h, aa, pal, aux, n_iterations)
        assert got.shape == (16 * 8, 4) and not got[4:].any()
        assert got[:4].tolist() == _colors_loop(frame, w, h, aa, pal, aux, n_iterations)


def test_saturating_frame_reaches_the_accumulator_maximum():
    pal = _current.saturating_palette()
    assert len(pal) == 7 and (65535, 0, 65535) in [tuple(e[:3]) for e in pal.tolist()]
    for aa in (1, 2, 3, 4):
        frame = _current.saturating_frame(70, 9, aa, np.uint32, 3)
        got = _current.colors(frame, 70 * aa, 9 * aa, aa, pal, 0, 2 ** 32 - 1)[:630, :3]
        assert got.tolist() == [e[:3] for e in _colors_loop(frame, 70 * aa, 9 * aa, aa, pal, 0, 2 ** 32 - 1)]
        pure = got.reshape(9, 70, 3)[np.add.outer(np.arange(9), np.arange(70)) % 2 == 0]
        assert set(map(tuple, pure.tolist())) == {tuple(e[:3]) for e in pal.tolist()}  # all sixteen samples on one entry


def test_injective_palette_is_injective():
    pal = _current.injective_palette(1 << 16)
    assert len(np.unique(pal[:, :2].astype(np.uint32) @ np.array([1, 1 << 16], np.uint32))) == 1 << 16
    big = np.arange(1 << 24, dtype=np.uint64)  # r, g of every index below 2^24, without building the 128 MiB palette
    key = (big & np.uint64(0xFFFF)) | (((big >> np.uint64(8)) & np.uint64(0xFFFF)) << np.uint64(16))
    assert len(np.unique(key)) == 1 << 24
    assert (pal[:, 3] == 0x1234).all()


def _reduction_loop(frame, w, rows, all_ones):
    mn, mx, s = all_ones, 0, 0
    for y in range(rows):
        for x in range(w):
            v = int(frame[y, x])
            mn, mx, s = min(mn, v), max(mx, v), s + v
    return mn, mx, s % 2 ** 64


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_reduction_against_a_plain_loop(dtype):
    all_ones = _current.ALL_ONES[np.dtype(dtype)]
    for w, rows in ((1, 1), (5, 3), (18, 9), (33, 17)):
        for name, frame in _current.reduction_frames(w, rows, dtype, 7):
            assert frame.shape == (_current.padded_rows(rows), _current.rounded_width(w))
            valid = frame[:rows, :w]
            assert valid.min() > 0 and valid.max() < all_ones  # strictly inside the poison values
            pad = np.ones(frame.shape, bool)
            pad[:rows, :w] = False
            assert set(frame[pad].tolist()) == {0, all_ones}
            assert _current.reduction(frame, w, rows, dtype) == _reduction_loop(frame, w, rows, all_ones), name
    assert _current.reduction(np.zeros((8, 16), dtype), 5, 0, dtype) == (all_ones, 0, 0)


def test_reduction_wraps_at_2_64():
    frame = _current.poisoned(np.array([[2 ** 64 - 2, 2 ** 63, 5]], np.uint64), np.uint64)
    assert _current.reduction(frame, 3, 1, np.uint64) == (5, 2 ** 64 - 2, (2 ** 64 - 2 + 2 ** 63 + 5) - 2 ** 64)
    name, frame = _current.reduction_frames(18, 40, np.uint64, 1)[0]
    true_sum = sum(int(v) for v in frame[:40, :18].ravel())
    assert true_sum > 2 ** 64 and _current.reduction(frame, 18, 40, np.uint64)[2] == true_sum % 2 ** 64


def test_reduction_positions_reach_every_path():
    """18 x 8209: every workgroup makes one four-rows trip, workgroups 0 .. 16 one tail trip; the places name one row of each."""
    assert _current.reduce_grid(18, 8209) == (1, 2048) and _current.reduce_grid(1030, 5) == (2, 5)
    assert _current.reduce_grid(2049, 2100) == (3, 683)
    pos = _current.reduction_positions(18, 8209)
    assert pos[:2] == [(0, 0), (8208, 17)] and len(set(pos)) == len(pos) == 7
    rows = [y for y, _ in pos[2:]]
    assert 2048 <= rows[0] < 4096 <= rows[1] < 6144 <= rows[2] < 8192 <= rows[3] < 8209 and rows[4] < 2048
    assert (rows[3], 17) in pos  # the last valid element of the partly valid group, in a tail trip
    assert _current.reduction_positions(1, 1) == [(0, 0)]


def _bands_loop(frame_rows, H, first, rows, stride, sentinel):
    local, image = [], []
    for y in range(H):
        own = rows == 0 or rows >= H or (y >= first and (y - first) % stride < rows)
        if own:
            local.append(frame_rows[y].tolist())
        image.append(frame_rows[y].tolist() if own else None)
    return local, image


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("cfg", _current.BAND_CONFIGS)
def test_bands_against_a_plain_loop(cfg, dtype):
    H, first, rows, stride = cfg
    rng = np.random.default_rng(H + first)
    frame = rng.integers(1, 2 ** 31, (H, 32), dtype=np.uint64).astype(dtype)
    local, image = _current.bands(frame, H, first, rows, stride, sentinel=0xA5)
    want_local, want_image = _bands_loop(frame, H, first, rows, stride, 0xA5)
    assert local.tolist() == want_local
    fill = int(np.frombuffer(b"\xa5" * 8, dtype)[0])
    assert image.tolist() == [r if r is not None else [fill] * 32 for r in want_image]
    counts = {(37, 8, 8, 24): 13, (40, 0, 8, 16): 24, (37, 0, 8, 16): 21, (20, 4, 6, 6): 16, (33, 30, 8, 8): 3, (37, 0, 0, 0): 37}
    assert len(local) == counts[cfg]


def test_case_keys_are_unique():
    keys = _current.case_keys()
    assert len(keys) == len(set(keys)) and len(keys) > 100
