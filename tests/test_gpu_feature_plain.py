"""fs_feature_eval_plain / fs_feature_eval_plain_direct, the Feature Finder's evaluators for T = float / double on the GPU: records
byte for byte against the CPU checker (tests/feature/feature_plain_ref.cpp) after every NaN in both has been replaced by one fixed
pattern (test_feature_plain_cpu.canonical), on the expanded and the waypoint-resident orbit; the whole scan through them against
the checker-backed scan, known answers, error codes, and no effect on the renderer's frame state.

Views: the fixture views shallow_1e-6 / -12 / -20 / -28 (tests/_truth.py), cap 20 000, the 12 x 12 grid.  The checker alone accepts
62 / 63 (f32 / f64), 73 / 66, 144 / 76 and - / 66 of the 144 candidates there; in float R^2 is subnormal at shallow_1e-20 (every
candidate triggers) and 0 at shallow_1e-28 (every candidate rejected: test_feature_plain_cpu)."""
import functools

import numpy as np
import pytest

from fractalshark_amd import GPURenderer, LAV2_FULL, T_F32, T_F64, T_HDR32, _capi, features, inputs
from fractalshark_amd.renderer import FS_ERR_UNSUPPORTED
from test_feature_finder_cpu import GRID, KNOWN, check_known, known_view
from test_feature_plain_cpu import (CAP, WAYPOINT_EXP, canonical, checker_direct_evaluator, checker_evaluator, first_batch,
                                    fixture_view)

pytestmark = pytest.mark.gpu

FS_ERR_6 = 10005
HIP_INVALID_VALUE = 1
TAG = {"f32": T_F32, "f64": T_F64}
ACCEPTING = [("shallow_1e-6", "f32"), ("shallow_1e-6", "f64"), ("shallow_1e-12", "f32"), ("shallow_1e-12", "f64"),
             ("shallow_1e-20", "f64"), ("shallow_1e-28", "f64")]


@functools.lru_cache(maxsize=None)
def plain_inputs(name, kind, compression_exp=None):
    v = fixture_view(name)
    return v, inputs.PlainInputs(v, kind, max_iter=CAP, compression_exp=compression_exp)


@functools.lru_cache(maxsize=None)
def find_round(name, kind, compression_exp=None):
    """(mode, R, records_in, the checker's records_out) of the view's first round; shared, never written to."""
    v, p = plain_inputs(name, kind, compression_exp)
    mode, radius, rin = first_batch(v, p, 4, CAP)
    assert mode == features.FIND
    cpu = np.zeros(len(rin), features.records_plain(kind == "f64")[1])
    checker_evaluator(p, 4, threads=16)(mode, radius, CAP, rin, cpu)
    for a in (radius, rin, cpu):
        a.setflags(write=False)
    return mode, radius, rin, cpu


def renderer_for(plain, waypoints=False):
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
    assert r.set_compressed_orbit_mode(waypoints) == 0
    assert r.InitializePerturbPlain(1, plain, with_la=False) == 0
    assert r.orbit_form == (2 if waypoints else 1)
    return r


def gpu_eval(r, kind, iter_bytes, mode, radius, cap, rin, direct=False):
    out = np.zeros(len(rin), features.records_plain(kind == "f64")[1])
    entry = r.FeatureEvalPlainDirect if direct else r.FeatureEvalPlain
    assert entry(TAG[kind], iter_bytes, mode, radius, cap, rin, out) == 0
    return out


def same(gpu, cpu):
    assert canonical(gpu) == canonical(cpu), "records differ at %s" % (np.nonzero(gpu != cpu)[0][:8],)


def both(r, plain, iter_bytes, mode, radius, cap, rin, waypoints=False):
    """fs_feature_eval_plain and the checker on the same records; equal under the comparison rule.  Returns the GPU's."""
    cpu = np.zeros(len(rin), features.records_plain(plain.kind == "f64")[1])
    checker_evaluator(plain, iter_bytes, threads=16, waypoints=waypoints)(mode, radius, cap, rin, cpu)
    gpu = gpu_eval(r, plain.kind, iter_bytes, mode, radius, cap, rin)
    same(gpu, cpu)
    return gpu


def fixed_at_found(rin, out):
    ok = out["status"] == features.OK
    fixed = rin[ok].copy()
    fixed["period"] = out["period"][ok]
    return fixed


@pytest.mark.parametrize("name,kind", ACCEPTING + [("shallow_1e-20", "f32")])
def test_find_then_fixed_bit_exact(name, kind):
    """The period search of the 144 grid points, then the fixed-period evaluation at each found period.  So that no comparison is
    of empty sets: the checker alone accepts at least 20 and (but at shallow_1e-20 in float, where R^2 is subnormal and the search
    lives on subnormal products: all 144 trigger) rejects at least 20."""
    v, p = plain_inputs(name, kind)
    mode, radius, rin, cpu = find_round(name, kind)
    accepted = int((cpu["status"] == features.OK).sum())
    assert accepted >= 20
    if (name, kind) != ("shallow_1e-20", "f32"):
        assert len(cpu) - accepted >= 20
    else:
        r2 = np.float32(radius[0]) * np.float32(radius[0])
        assert 0 < r2 < np.finfo(np.float32).tiny  # subnormal
    r = renderer_for(p)
    same(gpu_eval(r, kind, 4, features.FIND, radius, CAP, rin), cpu)
    fixed = fixed_at_found(rin, cpu)
    out = both(r, p, 4, features.FIXED, radius, CAP, fixed)
    assert (out["status"] == features.OK).all() and (out["period"] == fixed["period"]).all()
    r.close()


@pytest.mark.parametrize("name,kind", [("shallow_1e-12", "f32"), ("shallow_1e-6", "f32"), ("shallow_1e-12", "f64")])
def test_fixed_mode_takes_the_direct_fallback(name, kind):
    """The grid points that escaped in find mode, evaluated at the largest period the find round found: the PT evaluation escapes
    and PTEvaluator::Eval<false> goes on with Direct at T{cX_hp}.  In float that c is a different point (the view is far below
    binary32's resolution at 1e-12) which does not escape: FS_FEATURE_OK_DIRECT records; in double it is the same point and
    Direct escapes too (all rejected).  Equal on the GPU either way."""
    v, p = plain_inputs(name, kind)
    mode, radius, rin, cpu = find_round(name, kind)
    ok = cpu["status"] == features.OK
    fixed = rin[~ok].copy()
    fixed["period"] = cpu["period"][ok].max()
    r = renderer_for(p)
    out = both(r, p, 4, features.FIXED, radius, CAP, fixed)
    if kind == "f32":
        assert (out["status"] == features.OK_DIRECT).sum() >= 1
    r.close()


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_iter_bytes_and_slices(kind):
    """iter_bytes 4 and 8 give the same records; slices of 37 steps the records of the one-slice run; a fixed period of 2^32 is
    refused with a 4-byte IterType, not truncated."""
    v, p = plain_inputs("shallow_1e-12", kind)
    mode, radius, rin, cpu = find_round("shallow_1e-12", kind)
    r = renderer_for(p)
    one = gpu_eval(r, kind, 4, features.FIND, radius, CAP, rin)
    same(one, cpu)
    wide = both(r, p, 8, features.FIND, radius, CAP, rin)
    assert wide.tobytes() == one.tobytes()
    fixed = fixed_at_found(rin, cpu)
    whole = both(r, p, 4, features.FIXED, radius, CAP, fixed)
    assert r._lib.fs_set_feature_slice(r._h, 37) == 0
    assert gpu_eval(r, kind, 4, features.FIND, radius, CAP, rin).tobytes() == one.tobytes()
    assert gpu_eval(r, kind, 8, features.FIXED, radius, CAP, fixed).tobytes() == whole.tobytes()
    assert r._lib.fs_set_feature_slice(r._h, 0) == 0
    big = fixed[:2].copy()
    big["period"][1] = 1 << 32
    out = np.zeros(2, whole.dtype)
    assert r.FeatureEvalPlain(TAG[kind], 4, features.FIXED, radius, CAP, big, out) == HIP_INVALID_VALUE
    assert r.FeatureEvalPlainDirect(TAG[kind], 4, features.FIXED, radius, CAP, big, out) == HIP_INVALID_VALUE
    assert out.tobytes() == bytes(out.nbytes)
    r.close()


@pytest.mark.parametrize("iter_bytes", [4, 8])
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_waypoint_form(kind, iter_bytes):
    """The orbit held as its waypoints only: the records of the expanded form and of the checker's own decompressor, find and
    fixed, whole and in slices of 37 steps."""
    e = WAYPOINT_EXP[kind]
    v, p = plain_inputs("shallow_1e-12", kind, e)
    assert p.count == 1071 and 8 <= p.compressed_count < p.count // 8
    mode, radius, rin, cpu = find_round("shallow_1e-12", kind, e)
    assert (cpu["status"] == features.OK).sum() >= 20 and (cpu["status"] == features.REJECTED).sum() >= 20
    rx = renderer_for(p)
    expanded = gpu_eval(rx, kind, iter_bytes, features.FIND, radius, CAP, rin)
    same(expanded, cpu)
    fixed = np.concatenate([fixed_at_found(rin, cpu), rin[cpu["status"] == features.REJECTED][:8]])
    fixed["period"][-8:] = cpu["period"].max()  # (with the Direct fallback taken)
    expanded_fixed = gpu_eval(rx, kind, iter_bytes, features.FIXED, radius, CAP, fixed)
    rx.close()
    r = renderer_for(p, waypoints=True)
    for slice_steps in (0, 37):
        assert r._lib.fs_set_feature_slice(r._h, slice_steps) == 0
        out = both(r, p, iter_bytes, features.FIND, radius, CAP, rin, waypoints=True)
        assert out.tobytes() == expanded.tobytes()
        out = both(r, p, iter_bytes, features.FIXED, radius, CAP, fixed, waypoints=True)
        assert out.tobytes() == expanded_fixed.tobytes()
    r.close()


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_direct_view0(kind):
    """View 0 at 192 x 108, cap 8 192: the Direct period search of every pixel, then the fixed-period evaluation at the found
    periods, against the checker; a renderer fresh from fs_create."""
    v = inputs.View.builtin(0, 192, 108)
    rin, radius = features.direct_grid(v, kind == "f64", 192, 108, plain=True)
    dout = features.records_plain(kind == "f64")[1]
    cpu = np.zeros(len(rin), dout)
    checker_direct_evaluator(kind == "f64", 4, threads=16)(features.FIND, radius, 8192, rin, cpu)
    found = cpu["status"] == features.OK_DIRECT
    assert found.sum() >= 1000 and (~found).sum() >= 1000
    r = GPURenderer(0)
    same(gpu_eval(r, kind, 4, features.FIND, radius, 8192, rin, direct=True), cpu)
    fixed = rin[found].copy()
    fixed["period"] = cpu["period"][found]
    cpu_fixed = np.zeros(len(fixed), dout)
    checker_direct_evaluator(kind == "f64", 8, threads=16)(features.FIXED, radius, 8192, fixed, cpu_fixed)
    assert (cpu_fixed["status"] == features.OK_DIRECT).all()
    same(gpu_eval(r, kind, 8, features.FIXED, radius, 8192, fixed, direct=True), cpu_fixed)
    r.close()


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_period_map(kind):
    v = inputs.View.builtin(0, 64, 64)
    rin, radius = features.direct_grid(v, kind == "f64", 64, 64, plain=True)
    cpu = np.zeros(len(rin), features.records_plain(kind == "f64")[1])
    checker_direct_evaluator(kind == "f64", 4, threads=16)(features.FIND, radius, 1024, rin, cpu)
    want = np.where(cpu["status"] == features.OK_DIRECT, cpu["period"], 0).astype(np.uint64).reshape(64, 64)
    r = GPURenderer(0)
    got = features.period_map(r, v, 64, 64, T=TAG[kind], max_iters=1024)
    assert got.dtype == np.uint64 and np.array_equal(got, want) and len(np.unique(got)) > 3
    r.close()


@pytest.mark.parametrize("name,kind", [("shallow_1e-12", "f64"), ("shallow_1e-6", "f32")])
def test_whole_scan_matches_the_checker(name, kind):
    v, p = plain_inputs(name, kind)
    r = renderer_for(p)
    found = features.find_periodic_points(r, v, p, T=TAG[kind], iter_bytes=4, max_iters=CAP)
    assert found and found == features.scan(v, p, checker_evaluator(p, 4, threads=16), iter_bytes=4, max_iters=CAP)
    with pytest.raises(ValueError):  # a wrong pairing of T and orbit type
        features.find_periodic_points(r, v, p, T=T_F32 if kind == "f64" else T_F64)
    with pytest.raises(ValueError):
        features.find_periodic_points(r, v, p, T=T_HDR32)
    with pytest.raises(ValueError):
        features.find_periodic_points(r, v, inputs.Orbit(v), T=T_F32)
    r.close()


def test_whole_scan_on_waypoints_and_direct_scan():
    """find_periodic_points on a waypoint-resident plain orbit, and the DirectScan, each the checker-backed scan's found list."""
    e = WAYPOINT_EXP["f64"]
    v, p = plain_inputs("shallow_1e-12", "f64", e)
    r = renderer_for(p, waypoints=True)
    found = features.find_periodic_points(r, v, p, T=T_F64, max_iters=CAP)
    assert found and found == features.scan(v, p, checker_evaluator(p, 4, threads=16, waypoints=True), max_iters=CAP)
    r.close()
    centre, half, period = KNOWN[2]
    vk = known_view(centre, half)
    r = GPURenderer(0)
    found = features.find_periodic_points_direct(r, vk, nx=GRID, ny=GRID, T=T_F64)
    assert found == features.scan_direct(vk, True, checker_direct_evaluator(True, 4), nx=GRID, ny=GRID, plain=True)
    check_known(found, centre, period)
    r.close()


@pytest.mark.parametrize("centre,half,period", KNOWN)
def test_known_answers_through_the_gpu(centre, half, period):
    v = known_view(centre, half)
    p = inputs.PlainInputs(v, "f64")
    r = renderer_for(p)
    found = features.find_periodic_points(r, v, p, nx=GRID, ny=GRID, T=T_F64)
    assert found and found == features.scan(v, p, checker_evaluator(p, 4), nx=GRID, ny=GRID)
    check_known(found, centre, period)
    r.close()


def test_error_codes():
    v = known_view(*KNOWN[1][:2])
    p32, p64 = inputs.PlainInputs(v, "f32"), inputs.PlainInputs(v, "f64")
    rin, rout = np.zeros(1, features.FEATURE_IN_F32), np.zeros(1, features.FEATURE_OUT_F32)
    radius = np.full(1, 1e-3, np.float32)
    rin64, rout64, radius64 = np.zeros(1, features.FEATURE_IN_F64), np.zeros(1, features.FEATURE_OUT_F64), np.full(1, 1e-3)
    r = GPURenderer(0)
    # Direct needs nothing; the PT call needs an orbit
    assert r.FeatureEvalPlainDirect(T_F32, 4, features.FIND, radius, 16, rin, rout) == 0
    assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
    assert r.FeatureEvalPlain(T_F32, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_6  # no orbit
    assert r.InitializePerturbPlain(1, p32, with_la=False) == 0
    assert r.FeatureEvalPlain(T_F32, 4, features.FIND, radius, 16, rin, rout) == 0
    assert r.FeatureEvalPlain(T_F64, 4, features.FIND, radius64, 16, rin64, rout64) == FS_ERR_6  # no orbit of this type
    with pytest.raises(ValueError):  # records of the other type
        r.FeatureEvalPlain(T_F64, 4, features.FIND, radius, 16, rin, rout)
    for entry in (r.FeatureEvalPlain, r.FeatureEvalPlainDirect):
        for T in (2, 3, 4, 5, 6, 7, 8, -1):
            assert entry(T, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
        assert entry(T_F32, 4, 2, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED  # FS_FEATURE_LA
        assert entry(T_F32, 4, 3, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED  # unknown
        assert entry(T_F32, 2, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
        assert entry(T_F32, 4, features.FIND, radius, 16, rin[:0], rout[:0]) == 0  # n = 0
    lib, vp = r._lib, rin.ctypes.data
    for entry in (lib.fs_feature_eval_plain, lib.fs_feature_eval_plain_direct):
        for args in ((None, vp, rout.ctypes.data), (radius.ctypes.data, None, rout.ctypes.data), (radius.ctypes.data, vp, None)):
            assert entry(r._h, T_F32, 4, features.FIND, args[0], 16, args[1], args[2], 1) == HIP_INVALID_VALUE
    # the HDR calls keep refusing the plain tags and a plain orbit, the plain call an HDR orbit
    hin, hout, hrad = np.zeros(1, features.FEATURE_IN_HDR32), np.zeros(1, features.FEATURE_OUT_HDR32), np.zeros(1, features.REAL_HDR32)
    assert r.FeatureEval(T_HDR32, 4, features.FIND, hrad, 16, hin, hout) == FS_ERR_6
    assert r.FeatureEvalResident(T_HDR32, 4, features.FIND, hrad, 16, hin, hout) == FS_ERR_6
    assert r.FeatureEval(T_F32, 4, features.FIND, hrad, 16, hin, hout) == FS_ERR_UNSUPPORTED
    assert r.InitializePerturb(2, inputs.Orbit(v)) == 0
    assert r.FeatureEvalPlain(T_F32, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_6
    assert r.FeatureEval(T_HDR32, 4, features.FIND, hrad, 16, hin, hout) == 0
    assert r.InitializePerturbPlain(3, p64, with_la=False) == 0
    assert r.FeatureEvalPlain(T_F64, 8, features.FIXED, radius64, 16, rin64, rout64) == 0
    assert r.FeatureEvalPlain(T_F32, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_6
    r.close()


def test_set_up_rejects():
    """R <= 0 and cap < 1 reject in find mode; a fixed period of 0 is the reference's loop of no trips (Direct: all-zero values)."""
    v, p = plain_inputs("shallow_1e-12", "f32")
    mode, radius, rin, cpu = find_round("shallow_1e-12", "f32")
    r = renderer_for(p)
    for rad, cap in ((np.zeros(1, np.float32), CAP), (np.full(1, -1.0, np.float32), CAP), (radius, 0)):
        out = both(r, p, 4, features.FIND, rad, cap, rin[:70])
        assert out.tobytes() == bytes(out.nbytes)
    zero = rin[:3].copy()
    out = both(r, p, 4, features.FIXED, radius, CAP, zero)
    assert (out["status"] == features.OK_DIRECT).all() and (out["period"] == 0).all()
    r.close()


def test_scan_leaves_frame_state_alone():
    v, p = plain_inputs("shallow_1e-12", "f32")
    w, h = v.width * v.antialiasing, v.height * v.antialiasing
    r = GPURenderer(0)
    assert r.InitializeMemory(w, h, v.antialiasing, None, 0, 0, 0, False) == 0
    assert r.InitializePerturbPlain(1, p) == 0

    def frame():
        assert r.RenderPerturbLAv2Plain(p, v.num_iterations, Mode=LAV2_FULL) == 0
        out = r.new_iter_buffer()
        assert r.RenderCurrent(v.num_iterations, out, None, _capi.Reduction()) == 0
        assert r.SyncComputeStream() == 0
        return out.tobytes()

    before = frame()
    assert features.find_periodic_points(r, v, p, nx=4, ny=4, T=T_F32, max_iters=CAP)
    features.period_map(r, v, 8, 8, T=T_F32, max_iters=256)
    assert frame() == before
    r.close()
