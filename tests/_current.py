"""The device half of RenderCurrent as a reference model: antialias + palette (k_antialias), min / max / sum (k_reduce) and the
band copy (fs_copy_bands_to_host), in numpy and Python integers with no rounding anywhere; the synthetic frames and palettes
the tests feed both sides with; and the list of GPU cases, shared by tests/current/torch_current.py (which runs them) and
tests/test_gpu_current.py (which has one test per key)."""
import numpy as np

ALL_ONES = {np.dtype(np.uint32): 0xFFFFFFFF, np.dtype(np.uint64): 2 ** 64 - 1}
U32_CAP = 2 ** 32 - 1
U64_CAP = 2 ** 64 - 1
# fsk_reduce's grid (fractalshark_amd/csrc/kernels_current.hip): columns per block column, target number of workgroups
REDUCE_COLUMNS, REDUCE_WORKGROUPS = 1024, 2048


def rounded_width(w):
    return (w + 15) // 16 * 16


def padded_rows(rows):
    return (rows + 7) // 8 * 8


def color_elements(color_w, color_h):
    """fs_color_buffer_elements: the colour buffer is padded to 16 x 8 blocks of colour pixels."""
    return rounded_width(color_w) * padded_rows(color_h)


# ---- the model
def colors(frame, w, h, aa, pal, aux_depth, n_iterations):
    """antialiasing_kernel (AntialiasingKernel.cuh:3-71) over the valid w x h part of `frame`: per colour pixel the sums of r, g
    and b of pal[(n >> aux_depth) % len(pal)] over its aa x aa samples with n < n_iterations, integer-divided by aa * aa; alpha
    65535.  Laid out as RenderCurrent returns it: uint16[fs_color_buffer_elements, 4], dense rows of w / aa, the tail zero."""
    cw, ch = w // aa, h // aa
    n = np.ascontiguousarray(frame[:h, :w]).astype(np.uint64)
    live = n < np.uint64(n_iterations)
    idx = (n >> np.uint64(aux_depth)) % np.uint64(len(pal))
    rgb = pal[idx.astype(np.intp), :3].astype(np.uint64) * live[..., None].astype(np.uint64)
    acc = rgb.reshape(ch, aa, cw, aa, 3).sum(axis=(1, 3), dtype=np.uint64)
    out = np.zeros((color_elements(cw, ch), 4), np.uint16)
    out[:cw * ch, :3] = (acc // np.uint64(aa * aa)).reshape(cw * ch, 3)
    out[:cw * ch, 3] = 65535
    return out


def reduction(frame, w, rows, dtype):
    """(Min, Max, Sum) over the valid rows x w part only; Sum modulo 2^64; Min of nothing is the IterType's all-ones."""
    v = np.ascontiguousarray(frame[:rows, :w]).astype(np.uint64)
    if v.size == 0:
        return ALL_ONES[np.dtype(dtype)], 0, 0
    lo = int((v & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))  # < 2^32 terms of < 2^32 each: no wrap
    hi = int((v >> np.uint64(32)).sum(dtype=np.uint64))
    return int(v.min()), int(v.max()), ((hi << 32) + lo) % 2 ** 64


def owned_rows(H, first, rows, stride):
    """Frame rows a renderer owns under SetRowBands(first, rows, stride), in the order its local buffer holds them (the comment
    in compute_local_rows: band k covers [first + k stride, + rows), cut at the frame's edge); rows = 0 or >= H: no banding."""
    if rows == 0 or rows >= H:
        return list(range(H))
    out, start = [], first
    while start < H:
        out.extend(range(start, min(start + rows, H)))
        start += stride
    return out


def bands(frame_rows, H, first, rows, stride, sentinel=0xA5):
    """(local, image): the local buffer of the renderer that owns these bands of the frame `frame_rows` (its bands back to
    back), and what fs_copy_bands_to_host makes of an H-row host frame filled with the byte `sentinel`: the owned rows, whole
    pitch, in their places and nothing else touched."""
    own = owned_rows(H, first, rows, stride)
    local = np.ascontiguousarray(frame_rows[own])
    image = np.empty_like(frame_rows[:H])
    image.view(np.uint8)[...] = sentinel
    image[own] = local
    return local, image


# ---- palettes
def injective_palette(n):
    """Entry i = (i & 0xFFFF, (i >> 8) & 0xFFFF, (25173 i + 13849) & 0xFFFF, 0x1234): r and g together hold bits 0 .. 23 of i, so
    for n <= 2^24 no two entries are alike and at antialiasing 1 a wrong index always shows; the alpha is not 65535, so one
    copied from the palette shows too."""
    i = np.arange(n, dtype=np.uint64)
    pal = np.empty((n, 4), np.uint16)
    pal[:, 0] = i & np.uint64(0xFFFF)
    pal[:, 1] = (i >> np.uint64(8)) & np.uint64(0xFFFF)
    pal[:, 2] = (i * np.uint64(25173) + np.uint64(13849)) & np.uint64(0xFFFF)
    pal[:, 3] = 0x1234
    return pal


def saturating_palette():
    """Seven entries of 0 / 65535 per channel: at antialiasing 4 a group of sixteen (65535, ...) samples reaches the accumulator's
    maximum 16 x 65535, and (65535, 0, 65535) next to (0, 65535, 0) shows any bleed between the packed 16-bit fields."""
    m = 65535
    return np.array([(m, 0, m, 0x1234), (m, m, m, 0x1234), (0, m, 0, 0x1234), (0, 0, 0, 0x1234), (m, m, 0, 0x1234),
                     (0, 0, m, 0x1234), (0, m, m, 0x1234)], np.uint16)


# ---- frames
def poisoned(valid, dtype, extra_rows=0):
    """`valid` in the layout of the iteration buffer (rows of a multiple of 16 elements, a multiple of 8 rows, `extra_rows` more
    on request), the padding columns and rows alternating 0 and the IterType's all-ones: a reduction over values strictly
    between the two moves its Min, Max or Sum with any read of padding."""
    h, w = valid.shape
    H, W = padded_rows(h) + extra_rows, rounded_width(w)
    yy, xx = np.mgrid[0:H, 0:W]
    out = (((yy + xx) & 1).astype(dtype) * np.array(ALL_ONES[np.dtype(dtype)], dtype)).astype(dtype)
    out[:h, :w] = valid
    return out


def color_values(count, dtype, d, aux_depth, seed, cap=None):
    """`count` sample values for a colour frame whose palette has d entries: random over the whole type, and at random places the
    edges of the remainder -- 0, 1, d - 1, d, d + 1, k d - 1, k d, k d + 1 for the largest k that fits and some below it, 2^32 - 2,
    2^32 - 1 -- both as the sample itself and as the sample shifted down by aux_depth; for uint64 also values around 2^32 and
    2^63.  cap: an iteration limit, around which (cap - 2 .. cap + 2) a fifth of the samples then lie, so that coloured and
    uncoloured ones mix inside antialiasing groups."""
    dtype = np.dtype(dtype)
    top = ALL_ONES[dtype]
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, top, count, dtype=np.uint64, endpoint=True)
    edges = []
    for shift in sorted({0, aux_depth}):
        stop = top >> shift  # the largest shifted sample
        kmax = stop // d
        ks = sorted({k for k in (kmax, kmax - 1, kmax - 2, kmax - 3, kmax // 2, kmax // 3 + 1, 2, 1) if k >= 1})
        e = [0, 1, d - 1, d, d + 1, 2 ** 32 - 2, 2 ** 32 - 1, stop - 1, stop]
        for k in ks:
            e += [k * d - 1, k * d, k * d + 1]
        if dtype.itemsize == 8:
            e += [2 ** 32, 2 ** 32 + 1, 2 ** 32 + d, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 63 + d]
        low = (1 << shift) - 1
        for v in e:
            if 0 <= v <= stop:
                edges += [v << shift, (v << shift) | low]
    if cap is not None:
        near = rng.integers(-2, 2, count // 5, endpoint=True) + cap
        edges += [int(v) for v in near if 0 <= v <= top]
    edges = np.array(edges[:count], dtype=np.uint64)
    vals[rng.permutation(count)[:len(edges)]] = edges
    return vals.astype(dtype)


def color_frame(w, h, dtype, d, aux_depth, seed, cap=None, below=None):
    """A poisoned-padding frame of color_values; below: all random samples under this value (a low iteration limit)."""
    v = color_values(w * h, dtype, d, aux_depth, seed, cap)
    if below is not None:
        rng = np.random.default_rng(seed + 1)
        far = (v.astype(np.uint64) >= np.uint64(below))
        v[far] = rng.integers(0, below, int(far.sum()), dtype=np.uint64).astype(dtype)
    return poisoned(v.reshape(h, w), dtype)


def saturating_frame(cw, ch, aa, dtype, seed):
    """For saturating_palette: every other colour pixel has all its aa x aa samples on ONE palette entry (different multiples of
    7 plus the entry's index), so its sums are aa^2 x 65535 or 0 per channel; the pixels in between mix entries at random."""
    top = ALL_ONES[np.dtype(dtype)]
    rng = np.random.default_rng(seed)
    oy, ox = np.mgrid[0:ch * aa, 0:cw * aa] // aa
    entry = (ox + 3 * oy) % 7
    k = rng.integers(0, (top - 7) // 7, (ch * aa, cw * aa), dtype=np.uint64)
    one = k * np.uint64(7) + entry.astype(np.uint64)
    mixed = rng.integers(0, top, (ch * aa, cw * aa), dtype=np.uint64)
    return poisoned(np.where((ox + oy) % 2 == 0, one, mixed).astype(dtype), dtype)


def reduce_grid(w, rows):
    gx = (w + REDUCE_COLUMNS - 1) // REDUCE_COLUMNS
    return gx, min((REDUCE_WORKGROUPS + gx - 1) // gx, rows)


def reduction_positions(w, rows):
    """(y, x) places for a frame's one minimum and one maximum, each read by one code path of k_reduce only: the first element;
    the last valid one (the last of a partly valid group of four when w is no multiple of 4); a row read by the second, third
    and fourth load of a four-rows trip and one read in a tail trip, where the shape has them; in between, the last element of a
    full group of four."""
    gx, gy = reduce_grid(w, rows)
    loads = {0: [], 1: [], 2: [], 3: [], "tail": []}
    for by in range(gy):
        y = by
        while y + 3 * gy < rows:
            for k in range(4):
                loads[k].append(y + k * gy)
            y += 4 * gy
        while y < rows:
            loads["tail"].append(y)
            y += gy
    out = [(0, 0), (rows - 1, w - 1)]
    xs = [w // 2, (w - 1) // 4 * 4, min(3, w - 1), w - 1, 0]
    for i, key in enumerate((1, 2, 3, "tail", 0)):
        if loads[key]:
            out.append((loads[key][len(loads[key]) // 2], xs[i]))
    seen, uniq = set(), []
    for p in out:
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq


def reduction_background(w, rows, dtype, seed):
    """Random valid values strictly inside (1000, all-ones - 1000): room below for the one minimum and above for the one maximum."""
    top = ALL_ONES[np.dtype(dtype)]
    rng = np.random.default_rng(seed)
    return rng.integers(1001, top - 1001, (rows, w), dtype=np.uint64, endpoint=True).astype(dtype)


def reduction_frames(w, rows, dtype, seed):
    """[(name, frame in buffer layout with poisoned padding)]: the minimum 7 and the maximum all-ones - 1 walk through
    reduction_positions, and one frame is all equal."""
    top = ALL_ONES[np.dtype(dtype)]
    bg = reduction_background(w, rows, dtype, seed)
    pos = reduction_positions(w, rows)
    out = []
    for i, p in enumerate(pos):
        q = pos[(i + 1) % len(pos)]
        v = bg.copy()
        v[q] = top - 1
        v[p] = 7  # (a one-element frame: Min = Max = 7)
        out.append(("min%dx%d_max%dx%d" % (p + q), poisoned(v, dtype)))
    out.append(("all_equal", poisoned(np.full((rows, w), top - 1 if np.dtype(dtype).itemsize == 8 else 123456789, dtype), dtype)))
    return out


# ---- the GPU cases: key -> parameters (tests/current/torch_current.py runs them, tests/test_gpu_current.py lists them)
COLOR_W, COLOR_H = 70, 9  # the second 64-wide block has 6 live lanes, the third 4-row block one live wave
FAST_DIVISORS = (256, 257, 1792, 65536, 2 ** 24 - 1)
ABOVE_U32_CAP = 2 ** 32 + 1000


def _color(dtype, aa, pal_iters, aux=0, cap=None, n_iterations=None, size=(COLOR_W, COLOR_H), pal="injective", below=None,
           progressive=False):
    if n_iterations is None:
        n_iterations = U32_CAP if dtype == "uint32" else U64_CAP
    return dict(dtype=dtype, aa=aa, pal_iters=pal_iters, aux=aux, cap=cap, n_iterations=n_iterations, size=size, pal=pal,
                below=below, progressive=progressive)


def color_cases():
    c = {}
    for aa in (1, 4):  # every pal_iters at antialiasing 1 and 4; the two 128 MiB palettes at one of them each
        for p in (1, 7, 255, 256, 257, 1792, 65536):
            c["u32-aa%d-pal%d" % (aa, p)] = _color("uint32", aa, p)
    c["u32-aa4-pal%d" % 2 ** 24] = _color("uint32", 4, 2 ** 24)
    for aa in (2, 3):
        for p in (7, 1792):
            c["u32-aa%d-pal%d" % (aa, p)] = _color("uint32", aa, p)
    for aux in (1, 5, 31):
        c["u32-aa2-pal1792-aux%d" % aux] = _color("uint32", 2, 1792, aux)
    c["u32-aa3-pal7-aux5"] = _color("uint32", 3, 7, 5)
    c["u32-aa1-pal257-aux1"] = _color("uint32", 1, 257, 1)
    for aa in (1, 2, 3, 4):
        c["u32-aa%d-pal1792-cap1000" % aa] = _color("uint32", aa, 1792, cap=1000, n_iterations=1000, below=2000)
    for d in FAST_DIVISORS:  # about 65 000 samples through the device fast_mod, the edge set among them
        c["u32-aa1-pal%d-1024x64" % d] = _color("uint32", 1, d, size=(1024, 64))
    for aa in (1, 2, 3, 4):
        c["u32-aa%d-saturating" % aa] = _color("uint32", aa, 7, pal="saturating")
        for p in (7, 1792, 65536):
            c["u64-aa%d-pal%d" % (aa, p)] = _color("uint64", aa, p)
    for aux in (5, 33, 63):
        c["u64-aa2-pal1792-aux%d" % aux] = _color("uint64", 2, 1792, aux)
    c["u64-aa4-pal7-aux33"] = _color("uint64", 4, 7, 33)
    for aa in (1, 3):
        c["u64-aa%d-pal1792-cap_above_2^32" % aa] = _color("uint64", aa, 1792, cap=ABOVE_U32_CAP, n_iterations=ABOVE_U32_CAP,
                                                       below=2 * ABOVE_U32_CAP)
    c["u64-aa4-saturating"] = _color("uint64", 4, 7, pal="saturating")
    c["u32-aa4-pal1792-progressive"] = _color("uint32", 4, 1792, progressive=True)
    c["u64-aa2-pal65536-progressive"] = _color("uint64", 2, 65536, progressive=True)
    return c


def color_case_inputs(key, p):
    """(frame, w, h, palette) of a colour case; the seed is the case's own."""
    import zlib
    seed = zlib.crc32(key.encode())
    cw, ch = p["size"]
    w, h = cw * p["aa"], ch * p["aa"]
    if p["pal"] == "saturating":
        return saturating_frame(cw, ch, p["aa"], np.dtype(p["dtype"]), seed), w, h, saturating_palette()
    pal = injective_palette(p["pal_iters"])
    frame = color_frame(w, h, np.dtype(p["dtype"]), p["pal_iters"], p["aux"], seed, p["cap"], p["below"])
    return frame, w, h, pal


REDUCTION_SHAPES = {"uint32": ((18, 8209), (1030, 5), (1, 1), (16, 1), (4, 9), (2049, 2100)),
                    "uint64": ((18, 8209), (1030, 5), (1, 1), (16, 1), (4, 9))}
BAND_CONFIGS = ((37, 8, 8, 24), (40, 0, 8, 16), (37, 0, 8, 16), (20, 4, 6, 6), (33, 30, 8, 8), (37, 0, 0, 0))
BAND_W = 20


def case_keys():
    keys = ["color-" + k for k in color_cases()]
    keys += ["color-no_palette", "color-banded"]
    for dtype in ("uint32", "uint64"):
        keys += ["reduce-%s-%dx%d" % (dtype, w, rows) for w, rows in REDUCTION_SHAPES[dtype]]
        keys += ["reduce-%s-banded" % dtype, "reduce-%s-progressive" % dtype]
        for cfg in BAND_CONFIGS:
            for src in ("own", "device_iters"):
                keys.append("bands-%s-%d_%d_%d_%d-%s" % ((dtype,) + cfg + (src,)))
        for aa in (2, 4):
            for dst in ("tensor", "null"):
                keys.append("colorize-%s-aa%d-%s" % (dtype, aa, dst))
    keys.append("colorize-no_palette")
    return keys
