"""The Feature Finder's periodic-point scan (FeatureFinderOrchestrator PT / PTScan) with the evaluations batched on the GPU.

The reference walks its 12 x 12 grid of screen points one after another and runs, for each, a period search, up to 32 Newton
rounds and two final passes, every one a perturbation evaluation against the reference orbit on one CPU thread
(FeatureFinderOrchestrator.cpp:535-559, FeatureFinder.cpp:2443-2697).  Here the host keeps the high-precision state of every
candidate (libfsinputs: fsh_feature_*) and each round evaluates all candidates still running in one fs_feature_eval call, one
GPU lane per candidate (fs_feature_eval_resident where only the orbit's waypoints are resident).

The Direct / DirectScan modes (scan_direct, find_periodic_points_direct) are the same scan without a reference orbit, through
fs_feature_eval_direct; period_map is their period search alone over a dense grid of the view.  pt_grid makes the PT scan's
period-search round over a dense grid as records, without the state machine (the arguments of one fs_feature_eval call, which
sees a deep view where Direct sees one constant c); pt_axes the same grid as its four axes.

T is the reference's RenderAlg::MainType: HDRFloat<float> / HDRFloat<double> with an inputs.Orbit (T_HDR32 / T_HDR64), plain float /
double with an inputs.PlainInputs orbit (T_F32 / T_F64: fs_feature_eval_plain, fs_feature_eval_plain_direct) -- what the reference
runs for the Gpu1x32 / Gpu1x64 algorithms, its automatic choice for every zoom factor below 1e34.  In a plain T the squared search
radius underflows to 0 in a view narrow enough (float: below about 1e-21, double: about 1e-160) and the scan then finds nothing,
as the reference's does.
"""
import ctypes as C

import numpy as np

from . import _capi
from .renderer import T_F32, T_F64, T_HDR32, T_HDR64

FIND, FIXED = 0, 1  # FS_FEATURE_FIND / FS_FEATURE_FIXED
REJECTED, OK, OK_DIRECT = 0, 1, 2  # FS_FEATURE_* result status

_C32 = [("re", "<f4"), ("im", "<f4"), ("e", "<i4")]
_C64 = [("re", "<f8"), ("im", "<f8"), ("e", "<i4"), ("pad_", "<i4")]
FEATURE_IN_HDR32 = np.dtype([("dc", _C32), ("c", _C32), ("period", "<u8")])
FEATURE_IN_HDR64 = np.dtype([("dc", _C64), ("c", _C64), ("period", "<u8")])
FEATURE_OUT_HDR32 = np.dtype([("status", "<u4"), ("pad0_", "<u4"), ("period", "<u8"), ("diff", _C32), ("dzdc", _C32),
                              ("zcoeff", _C32), ("residual2", [("m", "<f4"), ("e", "<i4")]), ("pad1_", "<u4")])
FEATURE_OUT_HDR64 = np.dtype([("status", "<u4"), ("pad0_", "<u4"), ("period", "<u8"), ("diff", _C64), ("dzdc", _C64),
                              ("zcoeff", _C64), ("residual2", [("m", "<f8"), ("e", "<i4"), ("pad_", "<i4")])])
REAL_HDR32 = np.dtype([("m", "<f4"), ("e", "<i4")])
REAL_HDR64 = np.dtype([("m", "<f8"), ("e", "<i4"), ("pad_", "<i4")])
assert FEATURE_IN_HDR32.itemsize == 32 and FEATURE_IN_HDR64.itemsize == 56
assert FEATURE_OUT_HDR32.itemsize == 64 and FEATURE_OUT_HDR64.itemsize == 104
# T = float / double: {re, im} pairs (fs_feature_in_f32 / _f64, fs_feature_out_f32 / _f64); R is one float32 / float64
FEATURE_IN_F32 = np.dtype([("dc", "<f4", (2,)), ("c", "<f4", (2,)), ("period", "<u8")])
FEATURE_IN_F64 = np.dtype([("dc", "<f8", (2,)), ("c", "<f8", (2,)), ("period", "<u8")])
FEATURE_OUT_F32 = np.dtype([("status", "<u4"), ("pad0_", "<u4"), ("period", "<u8"), ("diff", "<f4", (2,)), ("dzdc", "<f4", (2,)),
                            ("zcoeff", "<f4", (2,)), ("residual2", "<f4"), ("pad1_", "<u4")])
FEATURE_OUT_F64 = np.dtype([("status", "<u4"), ("pad0_", "<u4"), ("period", "<u8"), ("diff", "<f8", (2,)), ("dzdc", "<f8", (2,)),
                            ("zcoeff", "<f8", (2,)), ("residual2", "<f8")])
assert FEATURE_IN_F32.itemsize == 24 and FEATURE_IN_F64.itemsize == 40
assert FEATURE_OUT_F32.itemsize == 48 and FEATURE_OUT_F64.itemsize == 72


def records(is64):
    """(input dtype, output dtype, radius dtype) of HDRFloat<float> (False) / HDRFloat<double> (True) evaluations."""
    return (FEATURE_IN_HDR64, FEATURE_OUT_HDR64, REAL_HDR64) if is64 else (FEATURE_IN_HDR32, FEATURE_OUT_HDR32, REAL_HDR32)


def records_plain(is64):
    """(input dtype, output dtype, radius dtype) of float (False) / double (True) evaluations."""
    return ((FEATURE_IN_F64, FEATURE_OUT_F64, np.dtype("<f8")) if is64 else
            (FEATURE_IN_F32, FEATURE_OUT_F32, np.dtype("<f4")))


def _plain_kind(orbit):
    """None for an inputs.Orbit; for an inputs.PlainInputs fsh_plain's kind, 0 float / 1 double (ValueError for "2x32": the
    reference leaves the CudaDblflt Feature Finder disabled)."""
    kind = getattr(orbit, "kind", None)
    if kind is None:
        return None
    if kind not in ("f32", "f64"):
        raise ValueError("no Feature Finder for PlainInputs of kind %r" % (kind,))
    return 0 if kind == "f32" else 1


def scan(view, orbit, evaluate, nx=12, ny=12, iter_bytes=4, max_iters=None):
    """The batched scan with any evaluator: evaluate(mode, radius, max_iters, records_in, records_out) fills records_out
    (fs_feature_eval's contract; fs_feature_eval_plain's for an inputs.PlainInputs orbit).  T follows the orbit.  Returns the found
    points in grid order (see find_periodic_points)."""
    lib = _capi.inputs_lib()
    n_iter = view.num_iterations if max_iters is None else int(max_iters)
    if _plain_kind(orbit) is None:
        h = lib.fsh_feature_begin(view._h, orbit._h, int(nx), int(ny), int(iter_bytes), n_iter)
    else:
        h = lib.fsh_feature_begin_plain(view._h, orbit._h, int(nx), int(ny), int(iter_bytes), n_iter)
    if not h:
        raise ValueError("fsh_feature_begin: bad arguments")
    return _run(lib, h, evaluate)


def _run(lib, h, evaluate):
    """The rounds of one fsh_feature scan, to its found points; destroys h."""
    try:
        kind = int(lib.fsh_feature_kind(h))
        din, dout, dreal = records_plain(kind == 3) if kind >= 2 else records(kind == 1)
        n_cand = int(lib.fsh_feature_candidates(h))
        rin, rout, rad = np.zeros(n_cand, din), np.zeros(n_cand, dout), np.zeros(1, dreal)
        mode, cap = C.c_int(0), C.c_uint64(0)
        while True:
            n = int(lib.fsh_feature_next_batch(h, rin.ctypes.data, n_cand, C.byref(mode), rad.ctypes.data, C.byref(cap)))
            if n == 0:
                break
            rout[:n] = np.zeros(n, dout)
            evaluate(mode.value, rad, cap.value, rin[:n], rout[:n])
            lib.fsh_feature_consume(h, rout.ctypes.data, n)
        found = []
        buf = [C.create_string_buffer(1 << 16) for _ in range(3)]
        period, r2, grid = C.c_uint64(0), np.zeros(1, REAL_HDR64), C.c_uint32(0)
        for k in range(int(lib.fsh_feature_found(h))):
            if lib.fsh_feature_result(h, k, buf[0], buf[1], buf[2], len(buf[0]), C.byref(period), r2.ctypes.data,
                                      C.byref(grid)) != 0:
                raise RuntimeError("fsh_feature_result failed")
            found.append({"grid": int(grid.value), "cx": buf[0].value.decode(), "cy": buf[1].value.decode(),
                          "period": int(period.value), "residual2": (float(r2["m"][0]), int(r2["e"][0])),
                          "intrinsic_radius": buf[2].value.decode()})
        return found
    finally:
        lib.fsh_feature_destroy(h)


def find_periodic_points(renderer, view, orbit, nx=12, ny=12, T=T_HDR32, iter_bytes=4, max_iters=None):
    """Periodic points near an nx x ny grid of the view's screen points (the reference's PTScan: 12 x 12), every evaluation on
    the GPU.  `renderer` must hold `orbit` (InitializePerturb; InitializePerturbPlain for an inputs.PlainInputs); T must be the
    orbit's type: T_HDR32 / T_HDR64 for an inputs.Orbit, T_F32 / T_F64 for an inputs.PlainInputs (ValueError otherwise).  A
    SimpleCompression orbit may be resident in either form: expanded, or as its waypoints only (renderer.orbit_form == 2, the one
    form an orbit of 2^32 and more entries fits in), which fs_feature_eval_resident / fs_feature_eval_plain walk with a cursor per
    candidate -- the same records either way.  max_iters: the period search's cap (default: the view's iteration limit).  Returns
    one dict per found point, in grid order: grid (row-major index), cx, cy (decimal strings), period, residual2
    (HDRFloat<double> as (mantissa, exponent)) and intrinsic_radius (decimal string)."""
    kind = _plain_kind(orbit)
    if kind is not None:
        if T != (T_F32, T_F64)[kind]:
            raise ValueError("T must be the orbit's type, T_F32 or T_F64")
        entry, name = renderer.FeatureEvalPlain, "fs_feature_eval_plain"
    else:
        if T not in (T_HDR32, T_HDR64) or (T == T_HDR64) != bool(orbit.is64):
            raise ValueError("T must be the orbit's type, T_HDR32 or T_HDR64")
        waypoints = renderer.orbit_form == 2
        entry, name = ((renderer.FeatureEvalResident, "fs_feature_eval_resident") if waypoints else
                       (renderer.FeatureEval, "fs_feature_eval"))

    def evaluate(mode, radius, cap, rin, rout):
        err = entry(T, iter_bytes, mode, radius, cap, rin, rout)
        if err:
            raise RuntimeError("%s failed: %d (%s)" % (name, err, renderer.ConvertErrorToString(err)))

    return scan(view, orbit, evaluate, nx, ny, iter_bytes, max_iters)


def scan_direct(view, is64, evaluate, nx=12, ny=12, iter_bytes=4, max_iters=None, at=None, plain=False):
    """The Direct / DirectScan modes with any evaluator (fs_feature_eval_direct's contract): no orbit; T = HDRFloat<double> when
    is64, else HDRFloat<float> -- with plain=True, double / float (fs_feature_eval_plain_direct's contract).  at = (px, py): the
    non-scan mode, one candidate (grid 0) at that screen point, nx and ny unused.
    Direct tells grid points apart only as far as T's mantissa does: far below its resolution every candidate is the same c."""
    lib = _capi.inputs_lib()
    n_iter = view.num_iterations if max_iters is None else int(max_iters)
    begin, begin_at = ((lib.fsh_feature_begin_plain_direct, lib.fsh_feature_begin_plain_direct_at) if plain else
                       (lib.fsh_feature_begin_direct, lib.fsh_feature_begin_direct_at))
    if at is None:
        h = begin(view._h, 1 if is64 else 0, int(nx), int(ny), int(iter_bytes), n_iter)
    else:
        h = begin_at(view._h, 1 if is64 else 0, int(at[0]), int(at[1]), int(iter_bytes), n_iter)
    if not h:
        raise ValueError("fsh_feature_begin_direct: bad arguments")
    return _run(lib, h, evaluate)


def _direct_evaluator(renderer, T, iter_bytes):
    if T not in (T_HDR32, T_HDR64, T_F32, T_F64):
        raise ValueError("T must be T_HDR32, T_HDR64, T_F32 or T_F64")
    entry, name = ((renderer.FeatureEvalPlainDirect, "fs_feature_eval_plain_direct") if T in (T_F32, T_F64) else
                   (renderer.FeatureEvalDirect, "fs_feature_eval_direct"))

    def evaluate(mode, radius, cap, rin, rout):
        err = entry(T, iter_bytes, mode, radius, cap, rin, rout)
        if err:
            raise RuntimeError("%s failed: %d (%s)" % (name, err, renderer.ConvertErrorToString(err)))

    return evaluate


def find_periodic_points_direct(renderer, view, nx=12, ny=12, T=T_HDR32, iter_bytes=4, max_iters=None):
    """The reference's DirectScan with every evaluation on the GPU: as find_periodic_points, without an orbit -- `renderer` needs
    none, nor InitializeMemory.  T = T_HDR32 / T_HDR64 / T_F32 / T_F64.  Returns the same dicts."""
    return scan_direct(view, T in (T_HDR64, T_F64), _direct_evaluator(renderer, T, iter_bytes), nx, ny, iter_bytes, max_iters,
                       plain=T in (T_F32, T_F64))


def direct_grid(view, is64, nx, ny, plain=False):
    """(records_in, radius) of a DirectScan's period-search round over the view's nx x ny grid points, row-major: the first batch
    of scan_direct, built without its state machine (libfsinputs does the high-precision arithmetic once per column and row)."""
    din, _, dreal = records_plain(is64) if plain else records(is64)
    rin, rad = np.zeros(int(nx) * int(ny), din), np.zeros(1, dreal)
    lib = _capi.inputs_lib()
    grid = lib.fsh_feature_plain_direct_grid if plain else lib.fsh_feature_direct_grid
    if grid(view._h, 1 if is64 else 0, int(nx), int(ny), rin.ctypes.data, rad.ctypes.data) != 0:
        raise ValueError("fsh_feature_direct_grid: bad arguments")
    return rin, rad


def _hdr_orbit_is64(orbit, what):
    """is64 of an inputs.Orbit; ValueError for an inputs.PlainInputs (the PT grid is built for the HDR types only)."""
    if getattr(orbit, "kind", None) is not None:
        raise ValueError("%s: an inputs.Orbit is needed, not an inputs.PlainInputs" % what)
    return bool(orbit.is64)


def pt_axes(view, orbit, nx, ny):
    """The find round of a PT scan over the view's nx x ny grid points as four axes: (dc_re[nx], dc_im[ny], c_re[nx], c_im[ny],
    radius) -- REAL_HDR32 / REAL_HDR64 records by the orbit's type, un-combined: grid point (gx, gy) has dc = C(dc_re[gx],
    dc_im[gy]) and c = C(c_re[gx], c_im[gy]), reduced: 2 (nx + ny) values describe the nx * ny records of pt_grid."""
    is64 = _hdr_orbit_is64(orbit, "pt_axes")
    dreal = records(is64)[2]
    nx, ny = int(nx), int(ny)
    if nx <= 0 or ny <= 0:
        raise ValueError("fsh_feature_pt_axes: bad arguments")
    ax = [np.zeros(n, dreal) for n in (nx, ny, nx, ny)]
    rad = np.zeros(1, dreal)
    if _capi.inputs_lib().fsh_feature_pt_axes(view._h, orbit._h, 1 if is64 else 0, nx, ny, *[a.ctypes.data for a in ax],
                                              rad.ctypes.data) != 0:
        raise ValueError("fsh_feature_pt_axes: bad arguments")
    return (*ax, rad)


def pt_grid(view, orbit, nx, ny):
    """(records_in, radius) of a PT scan's period-search round over the view's nx x ny grid points, row-major: the first batch of
    scan(view, orbit, ...), built without its state machine (the high-precision arithmetic once per column and row)."""
    is64 = _hdr_orbit_is64(orbit, "pt_grid")
    din, _, dreal = records(is64)
    nx, ny = int(nx), int(ny)
    if nx <= 0 or ny <= 0:
        raise ValueError("fsh_feature_pt_grid: bad arguments")
    rin, rad = np.zeros(nx * ny, din), np.zeros(1, dreal)
    if _capi.inputs_lib().fsh_feature_pt_grid(view._h, orbit._h, 1 if is64 else 0, nx, ny, rin.ctypes.data, rad.ctypes.data) != 0:
        raise ValueError("fsh_feature_pt_grid: bad arguments")
    return rin, rad


def period_map(renderer, view, nx, ny, T=T_HDR64, iter_bytes=4, max_iters=None):
    """The period the Direct search finds at each of the view's nx x ny grid points (the DirectScan's points and radius; nx = width,
    ny = height: every pixel), 0 where it finds none: a uint64 array (ny, nx).  The search round only -- one
    fs_feature_eval_direct (T_F32 / T_F64: fs_feature_eval_plain_direct) call, no Newton."""
    evaluate = _direct_evaluator(renderer, T, iter_bytes)
    plain, is64 = T in (T_F32, T_F64), T in (T_HDR64, T_F64)
    rin, rad = direct_grid(view, is64, nx, ny, plain)
    rout = np.zeros(len(rin), (records_plain if plain else records)(is64)[1])
    evaluate(FIND, rad, view.num_iterations if max_iters is None else int(max_iters), rin, rout)
    return np.where(rout["status"] == OK_DIRECT, rout["period"], 0).astype(np.uint64).reshape(int(ny), int(nx))


def _digits(n):
    """str(n) of an n >= 0 of any length (Python prints no more than 4300 digits in one go)."""
    chunk = 4000
    if n < 10 ** chunk:
        return str(n)
    parts = []
    while n:
        n, low = divmod(n, 10 ** chunk)
        parts.append(str(low).rjust(chunk, "0"))
    return "".join(reversed(parts)).lstrip("0")


def _decimal(v, frac_bits):
    """v / 2^frac_bits as an exact finite decimal string (v a Python integer)."""
    digits = _digits(abs(v) * 5 ** frac_bits).rjust(frac_bits + 1, "0")
    whole, frac = digits[:-frac_bits] if frac_bits else digits, (digits[-frac_bits:] if frac_bits else "").rstrip("0")
    return ("-" if v < 0 else "") + whole + ("." + frac if frac else "")


def refine_found(renderer, found, frac_bits=None, rounds=16, wide=False):
    """The points find_periodic_points returns, refined to nuclei of their period on the exact recurrence (DESIGN.md 6.3 "Point
    runs"): exact.refine_points with the GPU evaluator exact.eval_points (bailout 256, strict), every point started at its printed
    (cx, cy) with the offset delta = max(1, floor(intrinsic_radius * 2^F) >> 30), F = frac_bits (default exact.MAX_FRAC_BITS = 758;
    ValueError beyond).  wide=True: the evaluator is exact.eval_points(wide=True), a wave per run, and F goes up to
    exact.MAX_WIDE_FRAC_BITS = 22 518 (ValueError beyond); the results are the same wherever both run.  Needs no orbit and no
    InitializeMemory.  Returns one dict per point, in order: status ("fixed", "rounds",
    "stalled", "escaped"), c = (cx, cy) as integers c * 2^F and cx, cy as exact decimal strings (None where no iterate reached the
    period), atom (the atom period at c), converged (atom == period), period, evaluations, and log2 (log2 |z_p| of every iterate that
    reached the period, floats)."""
    from . import exact
    F = exact.MAX_FRAC_BITS if frac_bits is None else int(frac_bits)
    wide = bool(wide)
    if exact.limbs_for(F) > (exact.MAX_WIDE_LIMBS if wide else exact.MAX_LIMBS):
        raise ValueError("refine_found: %d fractional bits need more than %d limbs" % (F, exact.MAX_WIDE_LIMBS if wide else exact.MAX_LIMBS))
    cxs, _ = exact.points([p["cx"] for p in found], F)
    cys, _ = exact.points([p["cy"] for p in found], F)
    radii, _ = exact.points([p["intrinsic_radius"] for p in found], F)
    periods = [int(p["period"]) for p in found]
    res = exact.refine_points(lambda a, b, n: exact.eval_points(renderer, a, b, n, F, wide=wide), list(zip(cxs, cys)),
                              [max(1, r >> 30) for r in radii], periods, F, rounds)
    for q, p in zip(res, periods):
        q["period"] = p
        q["cx"], q["cy"] = (None, None) if q["c"] is None else (_decimal(q["c"][0], F), _decimal(q["c"][1], F))
    return res
