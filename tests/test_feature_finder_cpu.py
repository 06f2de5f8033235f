"""The Feature Finder scan (fsh_feature_*, fractalshark_amd.features.scan) with the CPU checker as its evaluator
(tests/feature/feature_ref.cpp), at shallow generated views whose periodic points are known: the scan starts off each nucleus and
must arrive on it, and every found point must be a root of z_p(c) to within 2^-30 |c| (2^-50 near c = 0), checked by an independent
mpmath iteration at 200 digits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fractalshark_amd import features, inputs

HERE = os.path.dirname(os.path.abspath(__file__))
FEATURE_DIR = os.path.join(HERE, "feature")
ROOT = os.path.dirname(HERE)


def checker_lib():
    """g++ build of tests/feature/feature_ref.cpp (which includes oracle/cpu_ref.cpp)."""
    lib = os.path.join(FEATURE_DIR, "libfeature_ref.so")
    srcs = [os.path.join(FEATURE_DIR, "feature_ref.cpp"), os.path.join(ROOT, "oracle", "cpu_ref.cpp"),
            os.path.join(ROOT, "include", "fs_layout.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", lib, srcs[0], "-lpthread"],
                       check=True)
    h = C.CDLL(lib)
    h.ffr_feature_eval.restype = None
    h.ffr_feature_eval.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                   C.c_void_p, C.c_uint64, C.c_int]
    return h


def checker_evaluator(orbit, iter_bytes, threads=1):
    lib = checker_lib()

    def evaluate(mode, radius, cap, rin, rout):
        radius = np.ascontiguousarray(radius)
        lib.ffr_feature_eval(1 if orbit.is64 else 0, iter_bytes, mode, radius.ctypes.data, cap, orbit.data_ptr, orbit.count,
                             rin.ctypes.data, rout.ctypes.data, len(rin), threads)
    return evaluate


# (nucleus, half-width of the view, period); nuclei to 30 digits
KNOWN = [(("0", "0"), "0.05", 1), (("-1", "0"), "0.05", 2),
         (("-0.122561166876653629174687877586", "0.744861766619744236593170428604"), "0.01", 3),
         (("-1.754877666246692760049508896358", "0"), "0.005", 3)]
GRID = 13  # odd: the middle grid point is the view's centre


def known_view(centre, half, size=96, iterations=2048, offset=(1 / 40, -1 / 50)):
    """A size x size view of width 2 half, its centre (the reference orbit's point and the middle point of an odd grid) moved from
    `centre` by offset x half: inside the middle point's search disc (a twelfth of the half-height), off the answer, so the period
    search and the Newton rounds have the way to the nucleus to go.  Bounds written with enough digits to keep the half-width, down
    to 1e-80."""
    import mpmath
    with mpmath.workdps(130):
        h = mpmath.mpf(half)
        x, y = mpmath.mpf(centre[0]) + offset[0] * h, mpmath.mpf(centre[1]) + offset[1] * h
        s = lambda v: mpmath.nstr(v, 120, strip_zeros=False)
        return inputs.View(s(x - h), s(y - h), s(x + h), s(y + h), size, size, iterations)


def known_orbit(view):
    """HDRFloat<double>: the binary32 mantissas of HDRFloat<float> leave Newton 2^-24 of |c| from the root, the bound of
    newton_ok is 2^-30."""
    return inputs.Orbit(view, is64=True)


def newton_ok(cx, cy, period, digits=200):
    """|z_p / z_p'| <= 2^-30 max(|c|, 2^-20) at c = cx + i cy (mpmath, `digits` decimal digits): relative to |c| as the reference's
    stop tests are, with an absolute floor of 2^-50 where c is near 0 (the period-1 nucleus), where a relative bound could only hold
    at c = 0 exactly."""
    import mpmath
    with mpmath.workdps(digits):
        c = mpmath.mpc(mpmath.mpf(cx), mpmath.mpf(cy))
        z, dz = mpmath.mpc(0), mpmath.mpc(0)
        for _ in range(period):
            dz = 2 * z * dz + 1
            z = z * z + c
        return abs(z / dz) <= mpmath.mpf(2) ** -30 * max(abs(c), mpmath.mpf(2) ** -20)


def check_known(found, centre, period):
    target = complex(float(centre[0]), float(centre[1]))
    near = [p for p in found if p["period"] == period and abs(complex(float(p["cx"]), float(p["cy"])) - target) < 1e-6]
    assert near, "no period-%d point near %r among %r" % (period, centre, [(p["period"], p["cx"][:12]) for p in found])
    for p in found:
        assert newton_ok(p["cx"], p["cy"], p["period"]), p


@pytest.mark.parametrize("centre,half,period", KNOWN)
def test_known_periodic_points_with_the_checker(centre, half, period):
    v = known_view(centre, half)
    ob = known_orbit(v)
    found = features.scan(v, ob, checker_evaluator(ob, 4), nx=GRID, ny=GRID)
    check_known(found, centre, period)


@pytest.mark.parametrize("centre,half,period", KNOWN)
def test_newton_moves_the_start_to_the_nucleus(centre, half, period):
    """The found point is the nucleus to within 1e-12, though the scan started 3 % of the half-width away from it."""
    import mpmath
    v = known_view(centre, half)
    ob = known_orbit(v)
    found = features.scan(v, ob, checker_evaluator(ob, 4), nx=GRID, ny=GRID)
    mid = [p for p in found if p["grid"] == GRID * GRID // 2]
    assert mid and mid[0]["period"] == period
    with mpmath.workdps(60):
        moved = abs(mpmath.mpc(mid[0]["cx"], mid[0]["cy"]) - mpmath.mpc(centre[0], centre[1]))
        start = abs(mpmath.mpc(1 / 40, -1 / 50) * mpmath.mpf(half))
    assert moved < mpmath.mpf("1e-12") < start


def test_batches_smaller_than_the_running_set():
    """fsh_feature_next_batch with a cap below the number of running candidates: every batch is of one mode, and the scan ends
    where the one-batch-per-round scan ends."""
    from fractalshark_amd import _capi
    v = known_view(*KNOWN[2][:2])
    ob = known_orbit(v)
    evaluate = checker_evaluator(ob, 4)
    lib = _capi.inputs_lib()
    h = lib.fsh_feature_begin(v._h, ob._h, GRID, GRID, 4, v.num_iterations)
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
    assert found == len(features.scan(v, ob, evaluate, nx=GRID, ny=GRID)) > 0


def test_scan_is_deterministic_and_in_grid_order():
    v = known_view(*KNOWN[2][:2])
    ob = inputs.Orbit(v)
    a = features.scan(v, ob, checker_evaluator(ob, 4), nx=5, ny=3)
    b = features.scan(v, ob, checker_evaluator(ob, 4, threads=4), nx=5, ny=3)
    assert a == b and a
    grids = [p["grid"] for p in a]
    assert grids == sorted(grids) and all(0 <= g < 15 for g in grids)
