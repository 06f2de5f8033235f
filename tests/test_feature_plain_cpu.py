"""CPU-only: the Feature Finder for the plain types T = float / double.  What fs_feature_eval_plain / fs_feature_eval_plain_direct add to
the C ABI; the scan (fsh_feature_begin_plain*, fractalshark_amd.features.scan) with the CPU checker as its evaluator
(tests/feature/feature_plain_ref.cpp) at views whose periodic points are known; the reference's underflow of the squared search
radius in float; and the compiled kernels' resources.  Also home of the helpers tests/test_gpu_feature_plain.py shares."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _truth
from fractalshark_amd import _capi, features, inputs
from test_feature_finder_cpu import GRID, KNOWN, check_known, known_view

HERE = os.path.dirname(os.path.abspath(__file__))
FEATURE_DIR = os.path.join(HERE, "feature")
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "feature_plain_parent_resources.json")
CAP = 20000
# SimpleCompression exponents at which the 1 071-entry orbit of shallow_1e-12 keeps a dozen or so waypoints (f32: 12, f64: 10):
# enough for the cursor to meet waypoints and long iterated stretches alike
WAYPOINT_EXP = {"f32": 6, "f64": 20}


def checker_lib():
    """g++ build of tests/feature/feature_plain_ref.cpp (which includes nothing of the project)."""
    lib = os.path.join(FEATURE_DIR, "libfeature_plain_ref.so")
    src = os.path.join(FEATURE_DIR, "feature_plain_ref.cpp")
    if not os.path.exists(lib) or os.path.getmtime(src) > os.path.getmtime(lib):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", lib, src, "-lpthread"], check=True)
    h = C.CDLL(lib)
    vp, u64 = C.c_void_p, C.c_uint64
    h.fpr_feature_eval.restype = None
    h.fpr_feature_eval.argtypes = [C.c_int, C.c_int, C.c_int, vp, u64, vp, u64, vp, u64, vp, vp, vp, u64, C.c_int]
    h.fpr_feature_eval_direct.restype = None
    h.fpr_feature_eval_direct.argtypes = [C.c_int, C.c_int, C.c_int, vp, u64, vp, vp, u64, C.c_int]
    return h


def checker_evaluator(plain, iter_bytes, threads=1, waypoints=False):
    """The checker as a features.scan evaluator on the orbit of `plain` (inputs.PlainInputs): the expanded entries, or -- waypoints
    -- its waypoints through the checker's own decompressor."""
    lib = checker_lib()
    is64 = 1 if plain.kind == "f64" else 0
    orbit = plain.orbit()
    wp = plain.waypoints() if waypoints else None
    low = plain.orbit_low() if waypoints else None

    def evaluate(mode, radius, cap, rin, rout):
        radius = np.ascontiguousarray(radius)
        if waypoints:
            lib.fpr_feature_eval(is64, iter_bytes, mode, radius.ctypes.data, cap, None, plain.count, wp.ctypes.data, len(wp),
                                 low.ctypes.data, rin.ctypes.data, rout.ctypes.data, len(rin), threads)
        else:
            lib.fpr_feature_eval(is64, iter_bytes, mode, radius.ctypes.data, cap, orbit.ctypes.data, plain.count, None, 0, None,
                                 rin.ctypes.data, rout.ctypes.data, len(rin), threads)
    return evaluate


def checker_direct_evaluator(is64, iter_bytes, threads=1):
    lib = checker_lib()

    def evaluate(mode, radius, cap, rin, rout):
        radius = np.ascontiguousarray(radius)
        lib.fpr_feature_eval_direct(1 if is64 else 0, iter_bytes, mode, radius.ctypes.data, cap, rin.ctypes.data, rout.ctypes.data,
                                    len(rin), threads)
    return evaluate


def canonical(records):
    """The records' bytes with every NaN replaced by one fixed pattern (host and device may make default NaNs that differ in sign
    or payload); every other bit, signed zeros and subnormals included, as it is."""
    r = records.copy()
    for name in ("diff", "dzdc", "zcoeff", "residual2"):
        f = r[name]
        f[np.isnan(f)] = np.nan
    return r.tobytes()


def first_batch(view, plain, iter_bytes, max_iters, grid=12):
    """The find-mode records of the view's grid x grid points, as the scan's first round makes them: (mode, R, records)."""
    recs = []

    def grab(mode, radius, cap, rin, rout):
        recs.append((mode, radius.copy(), rin.copy()))
        rout["status"] = features.REJECTED  # ends the scan after its first round

    features.scan(view, plain, grab, grid, grid, iter_bytes, max_iters)
    return recs[0]


def fixture_view(name):
    return _truth.Case(name).view(inputs)


def test_capi_declares_the_new_entries(native_libs):
    lib = _capi.render_lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    for name in ("fs_feature_eval_plain", "fs_feature_eval_plain_direct"):
        fn = getattr(lib, name)
        assert fn.restype is u32 and list(fn.argtypes) == [vp, C.c_int, u32, C.c_int, vp, u64, vp, vp, u64]
        assert name in _capi.RENDER_SYMBOLS
        assert hasattr(C.CDLL(native_libs.LIB_RENDER), name)
    public = open(os.path.join(ROOT, "include", "fsmi355.h")).read()
    assert re.search(r"uint32_t fs_feature_eval_plain\(fs_renderer \*r, int type_tag, uint32_t iter_bytes, int mode, "
                     r"const void \*radius,\s+uint64_t max_iters, const void \*in, void \*out, uint64_t n\);", public)
    assert re.search(r"uint32_t fs_feature_eval_plain_direct\(fs_renderer \*r, int type_tag, uint32_t iter_bytes, int mode, "
                     r"const void \*radius,\s+uint64_t max_iters, const void \*in, void \*out, uint64_t n\);", public)
    # the records: include/fs_layout.h static_asserts these sizes, _capi and features restate them
    sizes = {"in_f32": 24, "in_f64": 40, "out_f32": 48, "out_f64": 72}
    layout = open(os.path.join(ROOT, "include", "fs_layout.h")).read()
    for rec, size in sizes.items():
        assert re.search(r"sizeof\(fs_feature_%s\) == %d\b" % (rec, size), layout), rec
    assert [C.sizeof(t) for t in (_capi.FeatureInF32, _capi.FeatureInF64, _capi.FeatureOutF32, _capi.FeatureOutF64)] == \
        list(sizes.values())
    assert [d.itemsize for d in (features.FEATURE_IN_F32, features.FEATURE_IN_F64, features.FEATURE_OUT_F32,
                                 features.FEATURE_OUT_F64)] == list(sizes.values())
    inp = _capi.inputs_lib()
    for name in ("fsh_feature_begin_plain", "fsh_feature_begin_plain_direct", "fsh_feature_begin_plain_direct_at",
                 "fsh_feature_plain_direct_grid", "fsh_feature_kind"):
        assert getattr(inp, name).argtypes is not None, name


def test_the_scan_says_which_type_it_runs():
    lib = _capi.inputs_lib()
    v = known_view(*KNOWN[1][:2])
    kinds = []
    ob, p = inputs.Orbit(v), inputs.PlainInputs(v, "f32")
    for begin in (lambda: lib.fsh_feature_begin(v._h, ob._h, 3, 3, 4, 64),
                  lambda: lib.fsh_feature_begin_direct(v._h, 1, 3, 3, 4, 64),
                  lambda: lib.fsh_feature_begin_plain(v._h, p._h, 3, 3, 4, 64),
                  lambda: lib.fsh_feature_begin_plain_direct(v._h, 1, 3, 3, 4, 64)):
        h = begin()
        assert h
        kinds.append((lib.fsh_feature_kind(h), lib.fsh_feature_is64(h), lib.fsh_feature_candidates(h)))
        lib.fsh_feature_destroy(h)
    assert kinds == [(0, 0, 9), (1, 1, 9), (2, 0, 9), (3, 1, 9)]
    assert not lib.fsh_feature_begin_plain_direct(v._h, 2, 3, 3, 4, 64)  # kind is 0 or 1
    with pytest.raises(ValueError):
        features.scan(v, inputs.PlainInputs(v, "2x32"), None)


@pytest.mark.parametrize("centre,half,period", KNOWN)
def test_known_periodic_points_in_double(centre, half, period):
    v = known_view(centre, half)
    p = inputs.PlainInputs(v, "f64")
    found = features.scan(v, p, checker_evaluator(p, 4), nx=GRID, ny=GRID)
    check_known(found, centre, period)
    assert found == features.scan(v, p, checker_evaluator(p, 8, threads=4), nx=GRID, ny=GRID)


@pytest.mark.parametrize("centre,half,period", KNOWN)
def test_known_periods_in_float(centre, half, period):
    """float leaves Newton 2^-24 of |c| from the root, outside check_known's bound: the middle grid point's period only."""
    v = known_view(centre, half)
    p = inputs.PlainInputs(v, "f32")
    found = features.scan(v, p, checker_evaluator(p, 4), nx=GRID, ny=GRID)
    mid = [q for q in found if q["grid"] == GRID * GRID // 2]
    assert mid and mid[0]["period"] == period


def test_direct_scan_with_the_checker_finds_the_known_points():
    centre, half, period = KNOWN[2]
    v = known_view(centre, half)
    found = features.scan_direct(v, True, checker_direct_evaluator(True, 4), nx=GRID, ny=GRID, plain=True)
    check_known(found, centre, period)
    one = features.scan_direct(v, True, checker_direct_evaluator(True, 4), at=(48, 48), plain=True)
    assert [q["grid"] for q in one] == [0] and one[0]["period"] == period


def test_float_radius_underflows_at_1e28():
    """At shallow_1e-28 R is about 2e-30 and R * R = 0 in float: every candidate is rejected, as in the reference."""
    v = fixture_view("shallow_1e-28")
    p = inputs.PlainInputs(v, "f32", max_iter=CAP)
    mode, radius, rin = first_batch(v, p, 4, CAP)
    assert mode == features.FIND and len(rin) == 144 and radius.dtype == np.float32 and radius[0] == 0.0
    out = np.ones(len(rin), features.FEATURE_OUT_F32)
    checker_evaluator(p, 4)(mode, radius, CAP, rin, out)
    assert out.tobytes() == bytes(out.nbytes)
    assert features.scan(v, p, checker_evaluator(p, 4), max_iters=CAP) == []


def test_checker_cursor_path_equals_the_expanded_one():
    """The checker's own decompressor over the waypoints serves the orbit the host expanded: the same records."""
    v = fixture_view("shallow_1e-12")
    for kind, dout in (("f32", features.FEATURE_OUT_F32), ("f64", features.FEATURE_OUT_F64)):
        p = inputs.PlainInputs(v, kind, max_iter=CAP, compression_exp=WAYPOINT_EXP[kind])
        assert 8 <= p.compressed_count < p.count // 8
        mode, radius, rin = first_batch(v, p, 4, CAP)
        a, b = np.zeros(len(rin), dout), np.zeros(len(rin), dout)
        checker_evaluator(p, 4, threads=4)(mode, radius, CAP, rin, a)
        checker_evaluator(p, 8, threads=4, waypoints=True)(mode, radius, CAP, rin, b)
        assert (a["status"] == features.OK).sum() >= 20 and canonical(a) == canonical(b)


@pytest.fixture(scope="module")
def resources(native_libs):
    """{mangled kernel name: {vgpr, sgpr, scratch, lds}} of the built library (tools/kernel_resources.py --json)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--json"],
                         stdout=subprocess.PIPE, text=True, check=True).stdout
    table = json.loads(out)
    assert len(table) > 100
    return table


def test_new_kernels_use_no_scratch_and_no_lds(resources):
    """float | double x 4- / 8-byte IterType for the expanded, the waypoint and the Direct step kernel; the set-up kernels by
    lane record."""
    step = [k for k in resources if "k_featp_stepI" in k]
    seq = [k for k in resources if "k_featp_step_seqI" in k]
    direct = [k for k in resources if "k_featp_direct_stepI" in k]
    init = [k for k in resources if "k_featp_initI" in k]
    dinit = [k for k in resources if "k_featp_direct_initI" in k]
    assert [len(x) for x in (step, seq, direct, init, dinit)] == [4, 4, 4, 6, 2]
    assert sum("k_featp" in k for k in resources) == 20
    for k in step + seq + direct + init + dinit:
        assert resources[k]["scratch"] == 0 and resources[k]["lds"] == 0, (k, resources[k])
    # names that the counts of tests/test_feature_seq_cpu.py do not see
    assert not [k for k in resources if "k_featp" in k and ("k_feature_step_seqI" in k or "k_feature_initI" in k)]


def test_plain_render_kernels_compile_as_before(resources):
    """Every k_lav2_plain instantiation: VGPRs, SGPRs, scratch and LDS as on the parent commit (the plain cursor of
    kernels_plain.hip was left where it is; the Feature Finder's has positions as wide as the IterType and is its own text)."""
    parent = json.load(open(GOLDEN))["kernels"]
    assert len(parent) == 45
    mine = {k: v for k, v in resources.items() if "k_lav2_plainI" in k}
    assert sorted(mine) == sorted(parent)
    for name, want in parent.items():
        assert mine[name] == want, (name, mine[name], want)
