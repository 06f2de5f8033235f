"""fs_feature_eval, the Feature Finder's perturbation evaluator on the GPU: bit for bit against the CPU checker
(tests/feature/feature_ref.cpp), the whole scan through it against the checker-backed scan, known answers, error codes, and no
effect on the renderer's frame state."""
import json
import os

import numpy as np
import pytest

from fractalshark_amd import GPURenderer, LAV2_FULL, PARITY_CPU, T_HDR32, T_HDR64, _capi, features, inputs
from fractalshark_amd.renderer import FS_ERR_UNSUPPORTED
from test_feature_finder_cpu import GRID, KNOWN, check_known, checker_evaluator, known_orbit, known_view

pytestmark = pytest.mark.gpu

FS_ERR_6 = 10005
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_vectors.json")


def renderer_for(orbit, iter_bytes=4):
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
    assert r.InitializePerturb(1, orbit, iter_bytes=iter_bytes) == 0
    return r


def first_batch(view, orbit, iter_bytes, max_iters, grid=12):
    """The find-mode records of the view's grid x grid points, as the scan's first round makes them: (mode, R, records)."""
    recs = []

    def grab(mode, radius, cap, rin, rout):
        recs.append((mode, radius.copy(), rin.copy()))
        rout["status"] = features.REJECTED  # ends the scan after its first round

    features.scan(view, orbit, grab, grid, grid, iter_bytes, max_iters)
    return recs[0]


def both(r, orbit, T, iter_bytes, mode, radius, cap, rin):
    """fs_feature_eval and the checker on the same records; every output byte equal."""
    _, dout, _ = features.records(T == T_HDR64)
    gpu, cpu = np.zeros(len(rin), dout), np.zeros(len(rin), dout)
    assert r.FeatureEval(T, iter_bytes, mode, radius, cap, rin, gpu) == 0
    checker_evaluator(orbit, iter_bytes, threads=16)(mode, radius, cap, rin, cpu)
    assert gpu.tobytes() == cpu.tobytes(), "records differ at %s" % (np.nonzero(gpu != cpu)[0][:8],)
    return gpu


def find_then_fixed(r, view, orbit, T, iter_bytes, cap, grid=12):
    mode, radius, rin = first_batch(view, orbit, iter_bytes, cap, grid)
    assert mode == features.FIND
    out = both(r, orbit, T, iter_bytes, features.FIND, radius, cap, rin)
    ok = out["status"] == features.OK
    fixed = rin[ok].copy()
    fixed["period"] = out["period"][ok]
    if len(fixed):
        both(r, orbit, T, iter_bytes, features.FIXED, radius, cap, fixed)
    return out


@pytest.mark.parametrize("iter_bytes", [4, 8])
def test_view5_grid_bit_exact(iter_bytes):
    v = inputs.View.builtin(5, 192, 108)
    ob = inputs.Orbit(v)
    r = renderer_for(ob, iter_bytes)
    out = find_then_fixed(r, v, ob, T_HDR32, iter_bytes, 1 << 16)
    assert (out["status"] == features.OK).any()
    r.close()


def test_view14_grid_hdr64_bit_exact():
    v = inputs.View.builtin(14, 192, 108)
    ob = inputs.Orbit(v, max_iter=1 << 17, is64=True)
    r = renderer_for(ob)
    find_then_fixed(r, v, ob, T_HDR64, 4, 1 << 17)
    r.close()


def rabbit_nucleus(digits=150):
    """The period-3 nucleus near -0.1226 + 0.7449i to `digits` digits (mpmath Newton on z_3(c))."""
    import mpmath
    with mpmath.workdps(digits + 10):
        c = mpmath.mpc("-0.122561166876653629174687877586", "0.744861766619744236593170428604")
        for _ in range(12):
            z, dz = mpmath.mpc(0), mpmath.mpc(0)
            for _ in range(3):
                dz, z = 2 * z * dz + 1, z * z + c
            c -= z / dz
        return mpmath.nstr(c.real, digits, strip_zeros=False), mpmath.nstr(c.imag, digits, strip_zeros=False)


# from 1e-8 down to widths below binary32's range (2^-149 ~ 1.4e-45), around a nucleus so that the period search finds it from
# the middle grid point and the fixed-period step has records to compare
@pytest.mark.parametrize("half,T", [("1e-8", T_HDR32), ("1e-30", T_HDR32), ("1e-50", T_HDR32), ("1e-70", T_HDR64)])
def test_generated_views_bit_exact(half, T):
    v = known_view(rabbit_nucleus(), half, iterations=1 << 17)
    ob = inputs.Orbit(v, is64=(T == T_HDR64))
    r = renderer_for(ob)
    out = find_then_fixed(r, v, ob, T, 4, 1 << 17, grid=GRID)
    assert (out["status"] == features.OK).any()
    r.close()


def test_whole_scan_view5_matches_the_checker():
    """The reference's scan of View 5 at its iteration limit with every evaluation on the GPU: each round's records bit for bit
    equal to the checker's on the same inputs (the Direct fallback taken at full periods among them), the found points equal to
    the checker-backed scan's (tests/golden/feature_vectors.json)."""
    g = json.load(open(GOLDEN))
    v = inputs.View.builtin(5, g["width"], g["height"])
    ob = inputs.Orbit(v)
    r = renderer_for(ob)
    direct = []

    def evaluate(mode, radius, cap, rin, rout):
        out = both(r, ob, T_HDR32, 4, mode, radius, cap, rin)
        direct.extend(out["period"][out["status"] == features.OK_DIRECT].tolist())
        rout[:] = out

    found = features.scan(v, ob, evaluate, iter_bytes=4, max_iters=g["max_iters"])
    assert direct and min(direct) > 0
    assert found and [dict(p, residual2=list(p["residual2"])) for p in found] == g["found"]
    assert features.find_periodic_points(r, v, ob, T=T_HDR32, iter_bytes=4, max_iters=g["max_iters"]) == found
    r.close()


@pytest.mark.parametrize("centre,half,period", KNOWN)
def test_known_answers_through_the_gpu(centre, half, period):
    v = known_view(centre, half)
    ob = known_orbit(v)
    r = renderer_for(ob)
    found = features.find_periodic_points(r, v, ob, nx=GRID, ny=GRID, T=T_HDR64)
    assert found
    assert found == features.scan(v, ob, checker_evaluator(ob, 4), nx=GRID, ny=GRID)
    check_known(found, centre, period)
    r.close()


def test_error_codes():
    v = known_view(*KNOWN[1][:2])
    ob = inputs.Orbit(v)
    rin, rout = np.zeros(1, features.FEATURE_IN_HDR32), np.zeros(1, features.FEATURE_OUT_HDR32)
    radius = np.zeros(1, features.REAL_HDR32)
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
    assert r.FeatureEval(T_HDR32, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_6  # no orbit
    assert r.InitializePerturb(1, ob) == 0
    rin64, rout64 = np.zeros(1, features.FEATURE_IN_HDR64), np.zeros(1, features.FEATURE_OUT_HDR64)
    radius64 = np.zeros(1, features.REAL_HDR64)
    assert r.FeatureEval(T_HDR64, 4, features.FIND, radius64, 16, rin64, rout64) == FS_ERR_6  # no orbit of this type
    with pytest.raises(ValueError):  # records of the other type
        r.FeatureEval(T_HDR64, 4, features.FIND, radius, 16, rin, rout)
    for T in (0, 1, 2, 5, 6):
        assert r.FeatureEval(T, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
    assert r.FeatureEval(T_HDR32, 4, 2, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED  # LA mode
    assert r.FeatureEval(T_HDR32, 2, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
    assert r.FeatureEval(T_HDR32, 4, features.FIND, radius, 16, rin[:0], rout[:0]) == 0  # n = 0
    r.close()
    obc = inputs.Orbit(v, compression_exp=20)
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
    assert r._lib.fs_set_compressed_orbit_mode(r._h, 1) == 0
    assert r.InitializePerturb(1, obc) == 0
    assert r.FeatureEval(T_HDR32, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
    r.close()


def test_scan_leaves_frame_state_alone():
    v = inputs.View.builtin(5, 64, 36)
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False) == 0
    assert r.InitializePerturb(1, ob, 0, None, la) == 0
    co = [(float(c["m"]), int(c["e"])) for c in v.coords_perturb_hdr32(ob)]

    def frame():
        assert r.RenderPerturbLAv2(None, None, None, *co, v.num_iterations, T=T_HDR32, Mode=LAV2_FULL, parity=PARITY_CPU) == 0
        out = r.new_iter_buffer()
        assert r.RenderCurrent(v.num_iterations, out, None, _capi.Reduction()) == 0
        assert r.SyncComputeStream() == 0
        return out.tobytes()

    before = frame()
    features.find_periodic_points(r, v, ob, nx=4, ny=4, max_iters=1 << 16)
    assert frame() == before
    r.close()
