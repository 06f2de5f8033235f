"""The Feature Finder's periodic-point scan (FeatureFinderOrchestrator PT / PTScan) with the evaluations batched on the GPU.

The reference walks its 12 x 12 grid of screen points one after another and runs, for each, a period search, up to 32 Newton
rounds and two final passes, every one a perturbation evaluation against the reference orbit on one CPU thread
(FeatureFinderOrchestrator.cpp:535-559, FeatureFinder.cpp:2443-2697).  Here the host keeps the high-precision state of every
candidate (libfsinputs: fsh_feature_*) and each round evaluates all candidates still running in one fs_feature_eval call, one
GPU lane per candidate (fs_feature_eval_resident where only the orbit's waypoints are resident).

The Direct / DirectScan modes (scan_direct, find_periodic_points_direct) are the same scan without a reference orbit, through
fs_feature_eval_direct; period_map is their period search alone over a dense grid of the view.
"""
import ctypes as C

import numpy as np

from . import _capi
from .renderer import T_HDR32, T_HDR64

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


def records(is64):
    """(input dtype, output dtype, radius dtype) of HDRFloat<float> (False) / HDRFloat<double> (True) evaluations."""
    return (FEATURE_IN_HDR64, FEATURE_OUT_HDR64, REAL_HDR64) if is64 else (FEATURE_IN_HDR32, FEATURE_OUT_HDR32, REAL_HDR32)


def scan(view, orbit, evaluate, nx=12, ny=12, iter_bytes=4, max_iters=None):
    """The batched scan with any evaluator: evaluate(mode, radius, max_iters, records_in, records_out) fills records_out
    (fs_feature_eval's contract).  T follows the orbit.  Returns the found points in grid order (see find_periodic_points)."""
    lib = _capi.inputs_lib()
    n_iter = view.num_iterations if max_iters is None else int(max_iters)
    h = lib.fsh_feature_begin(view._h, orbit._h, int(nx), int(ny), int(iter_bytes), n_iter)
    if not h:
        raise ValueError("fsh_feature_begin: bad arguments")
    return _run(lib, h, evaluate)


def _run(lib, h, evaluate):
    """The rounds of one fsh_feature scan, to its found points; destroys h."""
    try:
        is64 = bool(lib.fsh_feature_is64(h))
        din, dout, dreal = records(is64)
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
    the GPU.  `renderer` must hold `orbit` (InitializePerturb); T must be the orbit's type.  A SimpleCompression orbit may be
    resident in either form: expanded, or as its waypoints only (renderer.orbit_form == 2, the one form an orbit of 2^32 and more
    entries fits in), which fs_feature_eval_resident walks with a cursor per candidate -- the same records either way.  max_iters:
    the period search's cap (default: the view's iteration limit).  Returns one dict per found point, in grid order: grid
    (row-major index), cx, cy (decimal strings), period, residual2 (HDRFloat<double> as (mantissa, exponent)) and
    intrinsic_radius (decimal string)."""
    if T not in (T_HDR32, T_HDR64) or (T == T_HDR64) != bool(orbit.is64):
        raise ValueError("T must be the orbit's type, T_HDR32 or T_HDR64")
    waypoints = renderer.orbit_form == 2
    entry, name = (renderer.FeatureEvalResident, "fs_feature_eval_resident") if waypoints else (renderer.FeatureEval, "fs_feature_eval")

    def evaluate(mode, radius, cap, rin, rout):
        err = entry(T, iter_bytes, mode, radius, cap, rin, rout)
        if err:
            raise RuntimeError("%s failed: %d (%s)" % (name, err, renderer.ConvertErrorToString(err)))

    return scan(view, orbit, evaluate, nx, ny, iter_bytes, max_iters)


def scan_direct(view, is64, evaluate, nx=12, ny=12, iter_bytes=4, max_iters=None, at=None):
    """The Direct / DirectScan modes with any evaluator (fs_feature_eval_direct's contract): no orbit; T = HDRFloat<double> when
    is64, else HDRFloat<float>.  at = (px, py): the non-scan mode, one candidate (grid 0) at that screen point, nx and ny unused.
    Direct tells grid points apart only as far as T's mantissa does: far below its resolution every candidate is the same c."""
    lib = _capi.inputs_lib()
    n_iter = view.num_iterations if max_iters is None else int(max_iters)
    if at is None:
        h = lib.fsh_feature_begin_direct(view._h, 1 if is64 else 0, int(nx), int(ny), int(iter_bytes), n_iter)
    else:
        h = lib.fsh_feature_begin_direct_at(view._h, 1 if is64 else 0, int(at[0]), int(at[1]), int(iter_bytes), n_iter)
    if not h:
        raise ValueError("fsh_feature_begin_direct: bad arguments")
    return _run(lib, h, evaluate)


def _direct_evaluator(renderer, T, iter_bytes):
    if T not in (T_HDR32, T_HDR64):
        raise ValueError("T must be T_HDR32 or T_HDR64")

    def evaluate(mode, radius, cap, rin, rout):
        err = renderer.FeatureEvalDirect(T, iter_bytes, mode, radius, cap, rin, rout)
        if err:
            raise RuntimeError("fs_feature_eval_direct failed: %d (%s)" % (err, renderer.ConvertErrorToString(err)))

    return evaluate


def find_periodic_points_direct(renderer, view, nx=12, ny=12, T=T_HDR32, iter_bytes=4, max_iters=None):
    """The reference's DirectScan with every evaluation on the GPU: as find_periodic_points, without an orbit -- `renderer` needs
    none, nor InitializeMemory.  Returns the same dicts."""
    return scan_direct(view, T == T_HDR64, _direct_evaluator(renderer, T, iter_bytes), nx, ny, iter_bytes, max_iters)


def direct_grid(view, is64, nx, ny):
    """(records_in, radius) of a DirectScan's period-search round over the view's nx x ny grid points, row-major: the first batch
    of scan_direct, built without its state machine (libfsinputs does the high-precision arithmetic once per column and row)."""
    din, _, dreal = records(is64)
    rin, rad = np.zeros(int(nx) * int(ny), din), np.zeros(1, dreal)
    if _capi.inputs_lib().fsh_feature_direct_grid(view._h, 1 if is64 else 0, int(nx), int(ny), rin.ctypes.data,
                                                  rad.ctypes.data) != 0:
        raise ValueError("fsh_feature_direct_grid: bad arguments")
    return rin, rad


def period_map(renderer, view, nx, ny, T=T_HDR64, iter_bytes=4, max_iters=None):
    """The period the Direct search finds at each of the view's nx x ny grid points (the DirectScan's points and radius; nx = width,
    ny = height: every pixel), 0 where it finds none: a uint64 array (ny, nx).  The search round only -- one
    fs_feature_eval_direct call, no Newton."""
    evaluate = _direct_evaluator(renderer, T, iter_bytes)
    rin, rad = direct_grid(view, T == T_HDR64, nx, ny)
    rout = np.zeros(len(rin), records(T == T_HDR64)[1])
    evaluate(FIND, rad, view.num_iterations if max_iters is None else int(max_iters), rin, rout)
    return np.where(rout["status"] == OK_DIRECT, rout["period"], 0).astype(np.uint64).reshape(int(ny), int(nx))
