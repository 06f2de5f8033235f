"""A dense PT grid without the state machine (fsh_feature_pt_axes, fsh_feature_pt_grid; features.pt_axes, features.pt_grid): the
grid as records is byte for byte the first batch of the scan's state machine, the radius too, and the four axes recombined on the
host -- C(re, im) reduced with hc_from_hr / hc_reduced of csrc/hdr_math.hpp (tests/feature/feature_axes_ref.cpp) -- give those
records' dc and c."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fractalshark_amd import _capi, features, inputs
from test_feature_finder_cpu import FEATURE_DIR, GRID, ROOT, known_view
from test_gpu_feature_finder import rabbit_nucleus

CAP = 1 << 17  # of the generated views, as tests/test_gpu_feature_finder.py has it


def view5():
    v = inputs.View.builtin(5, 192, 108)
    return v, inputs.Orbit(v)


def nucleus_view(half, is64):
    v = known_view(rabbit_nucleus(), half, iterations=CAP)
    return v, inputs.Orbit(v, is64=is64)


# name -> (view and orbit, grids (nx, ny))
CASES = {
    "view5": (view5, [(12, 12), (24, 13)]),
    "1e-30": (lambda: nucleus_view("1e-30", False), [(GRID, GRID)]),
    "1e-70": (lambda: nucleus_view("1e-70", True), [(GRID, GRID)]),
}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    make, grids = CASES[request.param]
    v, ob = make()
    return v, ob, grids


def scan_first_batch(view, orbit, nx, ny, iter_bytes=4, max_iters=CAP):
    """(mode, R, records) of the first round of features.scan over the nx x ny grid."""
    got = []

    def grab(mode, radius, cap, rin, rout):
        got.append((mode, radius.copy(), rin.copy()))
        rout["status"] = features.REJECTED  # ends the scan after this round

    features.scan(view, orbit, grab, nx, ny, iter_bytes, max_iters)
    return got[0]


def combiner():
    """g++ build of tests/feature/feature_axes_ref.cpp with libfsinputs' flags."""
    lib = os.path.join(FEATURE_DIR, "libfeature_axes_ref.so")
    srcs = [os.path.join(FEATURE_DIR, "feature_axes_ref.cpp"), os.path.join(ROOT, "fractalshark_amd", "csrc", "hdr_math.hpp"),
            os.path.join(ROOT, "include", "fs_layout.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", lib, srcs[0]], check=True)
    h = C.CDLL(lib)
    h.far_combine.restype = None
    h.far_combine.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    return h


def test_pt_grid_is_the_scans_first_batch(case):
    v, ob, grids = case
    for nx, ny in grids:
        mode, radius, want = scan_first_batch(v, ob, nx, ny)
        assert mode == features.FIND and len(want) == nx * ny
        rin, rad = features.pt_grid(v, ob, nx, ny)
        assert rin.dtype == want.dtype and rin.tobytes() == want.tobytes(), np.nonzero(rin != want)[0][:8]
        assert rad.dtype == radius.dtype and rad.tobytes() == radius.tobytes()
        assert (rin["period"] == 0).all()


def test_axes_recombine_to_the_records(case):
    v, ob, grids = case
    lib = combiner()
    for nx, ny in grids:
        rin, rad = features.pt_grid(v, ob, nx, ny)
        dc_re, dc_im, c_re, c_im, rad_axes = features.pt_axes(v, ob, nx, ny)
        assert [len(a) for a in (dc_re, dc_im, c_re, c_im)] == [nx, ny, nx, ny]
        assert rad_axes.tobytes() == rad.tobytes()
        for field, re, im in (("dc", dc_re, dc_im), ("c", c_re, c_im)):
            got = np.zeros(nx * ny, rin.dtype[field])
            lib.far_combine(1 if ob.is64 else 0, re.ctypes.data, nx, im.ctypes.data, ny, got.ctypes.data)
            assert got.tobytes() == np.ascontiguousarray(rin[field]).tobytes(), (field, nx, ny)


def test_deep_grid_points_differ_in_dc_only():
    """What a PT grid is for: at View 5 every grid point is one c in HDRFloat<float>, and dc tells them apart."""
    v, ob = view5()
    rin, _ = features.pt_grid(v, ob, 24, 13)
    assert len(np.unique(rin["c"])) == 1
    assert len(np.unique(rin["dc"])) == 24 * 13


def test_bad_arguments():
    v, ob = view5()
    lib = _capi.inputs_lib()
    din, _, dreal = features.records(False)
    rin, rad = np.zeros(4, din), np.zeros(1, dreal)
    ax = [np.zeros(2, dreal) for _ in range(4)]
    p = [a.ctypes.data for a in ax]
    assert lib.fsh_feature_pt_grid(v._h, ob._h, 0, 2, 2, rin.ctypes.data, rad.ctypes.data) == 0
    assert lib.fsh_feature_pt_axes(v._h, ob._h, 0, 2, 2, *p, rad.ctypes.data) == 0
    # NULL view, orbit, outputs; zero sizes; the other type than the orbit's
    assert lib.fsh_feature_pt_grid(None, ob._h, 0, 2, 2, rin.ctypes.data, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_grid(v._h, None, 0, 2, 2, rin.ctypes.data, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_grid(v._h, ob._h, 0, 2, 2, None, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_grid(v._h, ob._h, 0, 2, 2, rin.ctypes.data, None) == -1
    assert lib.fsh_feature_pt_grid(v._h, ob._h, 0, 0, 2, rin.ctypes.data, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_grid(v._h, ob._h, 0, 2, 0, rin.ctypes.data, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_grid(v._h, ob._h, 1, 2, 2, rin.ctypes.data, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_axes(None, ob._h, 0, 2, 2, *p, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_axes(v._h, None, 0, 2, 2, *p, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_axes(v._h, ob._h, 0, 0, 2, *p, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_axes(v._h, ob._h, 0, 2, 0, *p, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_axes(v._h, ob._h, 1, 2, 2, *p, rad.ctypes.data) == -1
    assert lib.fsh_feature_pt_axes(v._h, ob._h, 0, 2, 2, *p, None) == -1
    for k in range(4):
        q = list(p)
        q[k] = None
        assert lib.fsh_feature_pt_axes(v._h, ob._h, 0, 2, 2, *q, rad.ctypes.data) == -1
    with pytest.raises(ValueError):
        features.pt_grid(v, ob, 0, 3)
    with pytest.raises(ValueError):
        features.pt_axes(v, ob, 3, 0)


def test_plain_orbits_are_refused():
    class Plain:  # what features sees of an inputs.PlainInputs
        kind = "f32"

    v, _ = view5()
    for call in (features.pt_grid, features.pt_axes):
        with pytest.raises(ValueError):
            call(v, Plain(), 2, 2)
