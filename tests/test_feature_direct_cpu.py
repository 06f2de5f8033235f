"""The Feature Finder's Direct / DirectScan modes (fsh_feature_begin_direct, fractalshark_amd.features.scan_direct) with the CPU
checker as their evaluator (tests/feature/feature_direct_ref.cpp): the known nuclei of test_feature_finder_cpu, agreement with the
PT scan where both apply, the View 0 fixture, and the state machine's batching, determinism and order."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from fractalshark_amd import _capi, features, inputs
from test_feature_finder_cpu import GRID, KNOWN, check_known, checker_evaluator, known_orbit, known_view

HERE = os.path.dirname(os.path.abspath(__file__))
FEATURE_DIR = os.path.join(HERE, "feature")
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "feature_direct_vectors.json")


def direct_checker_lib():
    """g++ build of tests/feature/feature_direct_ref.cpp (which includes feature_ref.cpp and, through it, oracle/cpu_ref.cpp)."""
    lib = os.path.join(FEATURE_DIR, "libfeature_direct_ref.so")
    srcs = [os.path.join(FEATURE_DIR, "feature_direct_ref.cpp"), os.path.join(FEATURE_DIR, "feature_ref.cpp"),
            os.path.join(ROOT, "oracle", "cpu_ref.cpp"), os.path.join(ROOT, "include", "fs_layout.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", lib, srcs[0], "-lpthread"],
                       check=True)
    h = C.CDLL(lib)
    h.ffr_feature_eval_direct.restype = None
    h.ffr_feature_eval_direct.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.c_int]
    h.ffr_feature_eval_direct_steps.restype = None
    h.ffr_feature_eval_direct_steps.argtypes = h.ffr_feature_eval_direct.argtypes + [C.c_void_p]
    return h


def direct_checker_evaluator(is64, iter_bytes, threads=1):
    lib = direct_checker_lib()

    def evaluate(mode, radius, cap, rin, rout):
        radius = np.ascontiguousarray(radius)
        lib.ffr_feature_eval_direct(1 if is64 else 0, iter_bytes, mode, radius.ctypes.data, cap, rin.ctypes.data,
                                    rout.ctypes.data, len(rin), threads)
    return evaluate


def direct_first_batch(view, is64, iter_bytes, max_iters, nx=12, ny=12):
    """(mode, R, records) of a DirectScan's first round."""
    recs = []

    def grab(mode, radius, cap, rin, rout):
        recs.append((mode, radius.copy(), rin.copy()))
        rout["status"] = features.REJECTED  # ends the scan after its first round

    features.scan_direct(view, is64, grab, nx, ny, iter_bytes, max_iters)
    return recs[0]


def golden_view(g):
    return inputs.View.builtin(g["view"], g["width"], g["height"])


def as_json(found):
    return [dict(p, residual2=list(p["residual2"])) for p in found]


@pytest.mark.parametrize("centre,half,period", KNOWN)
def test_known_periodic_points_direct_hdr64(centre, half, period):
    v = known_view(centre, half)
    found = features.scan_direct(v, True, direct_checker_evaluator(True, 4), nx=GRID, ny=GRID)
    check_known(found, centre, period)


@pytest.mark.parametrize("centre,half,period", KNOWN)
def test_known_periodic_points_direct_hdr32_grid_and_period(centre, half, period):
    """HDRFloat<float>: the middle grid point finds the nucleus's period.  Not held to check_known's 2^-30: binary32 mantissas
    leave Newton 2^-24 of |c| from the root (the reason known_orbit is HDRFloat<double> for PT too)."""
    v = known_view(centre, half)
    found = features.scan_direct(v, False, direct_checker_evaluator(False, 4), nx=GRID, ny=GRID)
    mid = [p for p in found if p["grid"] == GRID * GRID // 2]
    assert mid and mid[0]["period"] == period


@pytest.mark.parametrize("centre,half,period", KNOWN)
def test_direct_and_pt_agree_at_known_views(centre, half, period):
    """Both modes find, from the same middle grid point, the same period."""
    v = known_view(centre, half)
    ob = known_orbit(v)
    pt = features.scan(v, ob, checker_evaluator(ob, 4), nx=GRID, ny=GRID)
    direct = features.scan_direct(v, True, direct_checker_evaluator(True, 4), nx=GRID, ny=GRID)
    mid = GRID * GRID // 2
    a = [(p["grid"], p["period"]) for p in pt if p["grid"] == mid]
    b = [(p["grid"], p["period"]) for p in direct if p["grid"] == mid]
    assert a == b == [(mid, period)]


def test_view0_scan_equals_the_fixture_and_is_not_pt():
    g = json.load(open(GOLDEN))
    v = golden_view(g)
    found = features.scan_direct(v, True, direct_checker_evaluator(True, 4), iter_bytes=4, max_iters=g["max_iters"])
    assert found and as_json(found) == g["found"]
    # the find round alone
    mode, radius, rin = direct_first_batch(v, True, 4, g["max_iters"])
    assert mode == features.FIND and (rin["dc"] == np.zeros(1, rin.dtype)["dc"]).all()
    rout = np.zeros(len(rin), features.FEATURE_OUT_HDR64)
    direct_checker_evaluator(True, 4)(mode, radius, g["max_iters"], rin, rout)
    periods = np.where(rout["status"] == features.OK_DIRECT, rout["period"], 0)
    assert periods.tolist() == g["find_periods"]
    assert set(np.unique(rout["status"])) == {features.REJECTED, features.OK_DIRECT}
    # Direct is not PT under another name: the fixed radius triggers where PeriodicityPP's tightened one does not
    ob = inputs.Orbit(v, is64=True)
    pt = features.scan(v, ob, checker_evaluator(ob, 4), iter_bytes=4, max_iters=g["max_iters"])
    assert len(found) > len(pt)


def test_direct_grid_records_equal_the_scans():
    """fsh_feature_direct_grid (period_map's records) = the first batch of fsh_feature_begin_direct, c and R, both T."""
    v = inputs.View.builtin(0, 192, 108)
    for is64 in (False, True):
        mode, radius, rin = direct_first_batch(v, is64, 4, 64)
        grin, grad = features.direct_grid(v, is64, 12, 12)
        assert grin.tobytes() == rin.tobytes() and grad.tobytes() == radius.tobytes()
        assert len(np.unique(grin["c"])) == 144
    with pytest.raises(ValueError):
        features.direct_grid(v, True, 0, 12)


def test_direct_batches_smaller_than_the_running_set():
    v = known_view(*KNOWN[2][:2])
    evaluate = direct_checker_evaluator(True, 4)
    lib = _capi.inputs_lib()
    h = lib.fsh_feature_begin_direct(v._h, 1, GRID, GRID, 4, v.num_iterations)
    assert h and lib.fsh_feature_is64(h) == 1 and lib.fsh_feature_candidates(h) == GRID * GRID
    din, dout, dreal = features.records(True)
    rin, rout, rad = np.zeros(7, din), np.zeros(7, dout), np.zeros(1, dreal)
    mode, cap, modes = C.c_int(0), C.c_uint64(0), []
    try:
        while True:
            n = int(lib.fsh_feature_next_batch(h, rin.ctypes.data, 7, C.byref(mode), rad.ctypes.data, C.byref(cap)))
            if n == 0:
                break
            assert (rin["period"][:n] == 0).all() == (mode.value == features.FIND)
            modes.append(mode.value)
            evaluate(mode.value, rad, cap.value, rin[:n], rout[:n])
            lib.fsh_feature_consume(h, rout.ctypes.data, n)
        found = int(lib.fsh_feature_found(h))
    finally:
        lib.fsh_feature_destroy(h)
    assert modes[:GRID * GRID // 7 + 1] == [features.FIND] * (GRID * GRID // 7 + 1)
    assert found == len(features.scan_direct(v, True, evaluate, nx=GRID, ny=GRID)) > 0


def test_direct_scan_is_deterministic_and_in_grid_order():
    v = known_view(*KNOWN[2][:2])
    for is64 in (False, True):
        a = features.scan_direct(v, is64, direct_checker_evaluator(is64, 4), nx=5, ny=3)
        b = features.scan_direct(v, is64, direct_checker_evaluator(is64, 4, threads=4), nx=5, ny=3)
        c = features.scan_direct(v, is64, direct_checker_evaluator(is64, 8, threads=3), nx=5, ny=3, iter_bytes=8)
        assert a == b == c and a
        grids = [p["grid"] for p in a]
        assert grids == sorted(grids) and all(0 <= g < 15 for g in grids)


def test_begin_direct_at_equals_the_grid_point_of_a_scan():
    """The non-scan Direct mode at the screen point of a grid cell = that cell's result in the scan (grid index aside)."""
    g = json.load(open(GOLDEN))
    v = golden_view(g)
    evaluate = direct_checker_evaluator(True, 4)
    scan = features.scan_direct(v, True, evaluate, max_iters=g["max_iters"])
    assert scan
    found_cells = {p["grid"] for p in scan}
    empty = next(k for k in range(144) if k not in found_cells)
    for p in scan[:3] + [{"grid": empty}]:
        gy, gx = divmod(p["grid"], 12)
        at = ((g["width"] * (2 * gx + 1)) // 24, (g["height"] * (2 * gy + 1)) // 24)
        one = features.scan_direct(v, True, evaluate, max_iters=g["max_iters"], at=at)
        assert one == ([dict(p, grid=0)] if len(p) > 1 else [])


def test_bad_arguments():
    v = inputs.View.builtin(0, 64, 36)
    lib = _capi.inputs_lib()
    assert not lib.fsh_feature_begin_direct(v._h, 1, 0, 12, 4, 16)
    assert not lib.fsh_feature_begin_direct(v._h, 1, 12, 12, 2, 16)
    assert not lib.fsh_feature_begin_direct_at(v._h, 0, 3, 3, 16, 16)
    with pytest.raises(ValueError):
        features.scan_direct(v, True, direct_checker_evaluator(True, 4), nx=0)
