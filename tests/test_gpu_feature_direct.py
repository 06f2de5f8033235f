"""fs_feature_eval_direct, the Feature Finder's Direct evaluator on the GPU: bit for bit, over whole record arrays, against the CPU
checker (tests/feature/feature_direct_ref.cpp); the DirectScan and the period map through it against the checker-backed ones and the
fixture; state carried across many short launches; error codes; no orbit needed and no effect on a renderer that has one.

Not tested: the reject of a trigger beyond what a 4-byte IterType holds (2^32 steps are out of a test's reach); checker and
kernel both restate it."""
import json
import os

import numpy as np
import pytest

from fractalshark_amd import GPURenderer, LAV2_FULL, PARITY_CPU, T_HDR32, T_HDR64, _capi, features, inputs
from fractalshark_amd.renderer import FS_ERR_UNSUPPORTED
from test_feature_direct_cpu import (GOLDEN, as_json, direct_checker_evaluator, direct_checker_lib, direct_first_batch,
                                     golden_view)
from test_feature_finder_cpu import GRID, checker_evaluator, known_view
from test_gpu_feature_finder import first_batch, rabbit_nucleus

pytestmark = pytest.mark.gpu

BOTH_T = [T_HDR32, T_HDR64]


def bare_renderer(init_memory=True):
    """A renderer that is never given an orbit."""
    r = GPURenderer(0)
    if init_memory:
        assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
    return r


def both(r, T, iter_bytes, mode, radius, cap, rin):
    """fs_feature_eval_direct and the checker on the same records; every output byte equal."""
    is64 = T == T_HDR64
    _, dout, _ = features.records(is64)
    gpu, cpu = np.zeros(len(rin), dout), np.zeros(len(rin), dout)
    gpu["status"] = 77  # (every record must be written)
    assert r.FeatureEvalDirect(T, iter_bytes, mode, radius, cap, rin, gpu) == 0
    direct_checker_evaluator(is64, iter_bytes, threads=16)(mode, radius, cap, rin, cpu)
    assert gpu.tobytes() == cpu.tobytes(), "records differ at %s" % (np.nonzero(gpu != cpu)[0][:8],)
    return gpu


def find_then_fixed(r, view, T, iter_bytes, cap, nx=12, ny=12, short_slices=False):
    """The view's period-search round, then the fixed-period evaluation of what it found.  short_slices: both once more with 64
    steps per launch, which must change nothing."""
    mode, radius, rin = direct_first_batch(view, T == T_HDR64, iter_bytes, cap, nx, ny)
    assert mode == features.FIND
    out = both(r, T, iter_bytes, features.FIND, radius, cap, rin)
    assert set(np.unique(out["status"])) <= {features.REJECTED, features.OK_DIRECT}
    ok = out["status"] == features.OK_DIRECT
    fixed = rin[ok].copy()
    fixed["period"] = out["period"][ok]
    fout = both(r, T, iter_bytes, features.FIXED, radius, cap, fixed) if len(fixed) else None
    if short_slices:
        assert r._lib.fs_set_feature_slice(r._h, 64) == 0
        assert both(r, T, iter_bytes, features.FIND, radius, cap, rin).tobytes() == out.tobytes()
        if len(fixed):
            assert both(r, T, iter_bytes, features.FIXED, radius, cap, fixed).tobytes() == fout.tobytes()
        assert r._lib.fs_set_feature_slice(r._h, 0) == 0
    return out


def checker_steps(is64, radius, cap, rin):
    """Loop trips per candidate of the period search (the checker's count)."""
    lib = direct_checker_lib()
    out, steps = np.zeros(len(rin), features.records(is64)[1]), np.zeros(len(rin), np.uint64)
    lib.ffr_feature_eval_direct_steps(1 if is64 else 0, 4, features.FIND, np.ascontiguousarray(radius).ctypes.data, cap,
                                      rin.ctypes.data, out.ctypes.data, len(rin), 16, steps.ctypes.data)
    return steps


@pytest.mark.parametrize("iter_bytes", [4, 8])
@pytest.mark.parametrize("T", BOTH_T)
def test_view0_find_then_fixed_without_an_orbit(T, iter_bytes):
    v = inputs.View.builtin(0, 192, 108)
    r = bare_renderer()
    out = find_then_fixed(r, v, T, iter_bytes, 8192)
    # not a vacuous pass: triggers and rejects both present
    assert (out["status"] == features.OK_DIRECT).any() and (out["status"] == features.REJECTED).any()
    assert (out["period"][out["status"] == features.OK_DIRECT] > 0).all()
    r.close()


def test_without_initialize_memory():
    v = inputs.View.builtin(0, 192, 108)
    r = bare_renderer(init_memory=False)
    out = find_then_fixed(r, v, T_HDR64, 4, 8192)
    assert (out["status"] == features.OK_DIRECT).any()
    r.close()


@pytest.mark.parametrize("T", BOTH_T)
def test_view5_long_runs_bit_exact(T):
    """Far below T's resolution all 144 candidates are one c: nothing to find, but long runs (HDRFloat<float>: 60 030 steps) to
    compare."""
    v = inputs.View.builtin(5, 192, 108)
    r = bare_renderer()
    out = find_then_fixed(r, v, T, 4, 1 << 16, short_slices=True)  # (a fixed period of ~ 940 launches at 64 steps each)
    assert len(np.unique(out["status"])) == 1
    r.close()


@pytest.mark.parametrize("half", ["1e-8", "1e-30"])
@pytest.mark.parametrize("T", BOTH_T)
def test_generated_views_bit_exact(half, T):
    v = known_view(rabbit_nucleus(), half, iterations=1 << 17)
    r = bare_renderer()
    find_then_fixed(r, v, T, 4, 1 << 17, GRID, GRID, short_slices=True)
    r.close()


@pytest.mark.parametrize("T", BOTH_T)
def test_dense_grid_default_and_short_slices(T):
    """128 x 128 candidates: the lanes of a wave finish at different steps; with 64 steps per launch they finish in different
    launches, their state carried in device memory.  Same records either way."""
    v = inputs.View.builtin(0, 512, 512)
    mode, radius, rin = direct_first_batch(v, T == T_HDR64, 4, 8192, 128, 128)
    assert len(rin) == 128 * 128
    r = bare_renderer()
    out = both(r, T, 4, features.FIND, radius, 8192, rin)
    assert (out["status"] == features.OK_DIRECT).any() and (out["status"] == features.REJECTED).any()
    # the premise: in one and the same wave, lanes that end within the first 64 steps beside lanes that need many launches
    steps = checker_steps(T == T_HDR64, radius, 8192, rin).reshape(-1, 64)
    assert ((steps.min(axis=1) <= 64) & (steps.max(axis=1) > 64 * 16)).any()
    assert r._lib.fs_set_feature_slice(r._h, 64) == 0
    short = both(r, T, 4, features.FIND, radius, 8192, rin)
    assert short.tobytes() == out.tobytes()
    ok = out["status"] == features.OK_DIRECT
    fixed = rin[ok].copy()
    fixed["period"] = out["period"][ok]
    a = both(r, T, 4, features.FIXED, radius, 8192, fixed)
    assert r._lib.fs_set_feature_slice(r._h, 0) == 0
    assert both(r, T, 4, features.FIXED, radius, 8192, fixed).tobytes() == a.tobytes()
    r.close()


def test_scan_view0_matches_fixture_and_checker():
    g = json.load(open(GOLDEN))
    v = golden_view(g)
    r = bare_renderer()
    found = features.find_periodic_points_direct(r, v, T=T_HDR64, iter_bytes=4, max_iters=g["max_iters"])
    assert found and as_json(found) == g["found"]
    assert found == features.scan_direct(v, True, direct_checker_evaluator(True, 4), max_iters=g["max_iters"])
    # every round's records, not only the result
    rounds = []

    def evaluate(mode, radius, cap, rin, rout):
        rout[:] = both(r, T_HDR64, 4, mode, radius, cap, rin)
        rounds.append(mode)

    assert features.scan_direct(v, True, evaluate, max_iters=g["max_iters"]) == found
    assert rounds[0] == features.FIND and features.FIXED in rounds
    # HDRFloat<float>: equal to its own checker-backed scan
    f32 = features.find_periodic_points_direct(r, v, T=T_HDR32, max_iters=g["max_iters"])
    assert f32 and f32 == features.scan_direct(v, False, direct_checker_evaluator(False, 4), max_iters=g["max_iters"])
    r.close()


def test_period_map():
    g = json.load(open(GOLDEN))
    v = golden_view(g)
    r = bare_renderer()
    m = features.period_map(r, v, 12, 12, max_iters=g["max_iters"])
    assert m.dtype == np.uint64 and m.shape == (12, 12) and m.ravel().tolist() == g["find_periods"]
    v = inputs.View.builtin(0, 256, 256)
    for T in BOTH_T:
        m = features.period_map(r, v, 256, 256, T=T, max_iters=2048)
        rin, rad = features.direct_grid(v, T == T_HDR64, 256, 256)
        out = both(r, T, 4, features.FIND, rad, 2048, rin)
        ref = np.where(out["status"] == features.OK_DIRECT, out["period"], 0).reshape(256, 256)
        assert (m == ref).all() and (m != 0).any() and (m == 0).any()
    r.close()


def test_leaves_frame_orbit_and_pt_evaluator_alone():
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

    mode, radius, rin = first_batch(v, ob, 4, 1 << 14, 4)

    def pt():
        out = np.zeros(len(rin), features.FEATURE_OUT_HDR32)
        assert r.FeatureEval(T_HDR32, 4, mode, radius, 1 << 14, rin, out) == 0
        return out.tobytes()

    frame_before, pt_before = frame(), pt()
    ref = np.zeros(len(rin), features.FEATURE_OUT_HDR32)
    checker_evaluator(ob, 4)(mode, radius, 1 << 14, rin, ref)
    assert pt_before == ref.tobytes()
    v0 = inputs.View.builtin(0, 192, 108)
    assert features.find_periodic_points_direct(r, v0, T=T_HDR32, max_iters=8192)
    assert features.find_periodic_points_direct(r, v0, T=T_HDR64, max_iters=8192)
    assert features.period_map(r, v0, 64, 64, max_iters=1024).any()
    assert frame() == frame_before
    assert pt() == pt_before
    r.close()


def test_error_codes():
    r = bare_renderer()
    rin, rout = np.zeros(1, features.FEATURE_IN_HDR32), np.zeros(1, features.FEATURE_OUT_HDR32)
    radius = np.zeros(1, features.REAL_HDR32)
    for T in (0, 1, 2, 5, 6):
        assert r.FeatureEvalDirect(T, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
    assert r.FeatureEvalDirect(T_HDR32, 4, 2, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED  # LA mode
    assert r.FeatureEvalDirect(T_HDR32, 4, -1, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
    for iter_bytes in (0, 2, 16):
        assert r.FeatureEvalDirect(T_HDR32, iter_bytes, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
    with pytest.raises(ValueError):  # records of the other type
        r.FeatureEvalDirect(T_HDR64, 4, features.FIND, radius, 16, rin, rout)
    assert r.FeatureEvalDirect(T_HDR32, 4, features.FIND, radius, 16, rin[:0], rout[:0]) == 0  # n = 0
    assert r.FeatureEvalDirect(T_HDR64, 8, features.FIXED, np.zeros(1, features.REAL_HDR64),
                               16, np.zeros(0, features.FEATURE_IN_HDR64), np.zeros(0, features.FEATURE_OUT_HDR64)) == 0
    wide = rin.copy()
    wide["period"] = 1 << 32  # a fixed period that a 4-byte IterType cannot hold: refused, not truncated
    assert r.FeatureEvalDirect(T_HDR32, 4, features.FIXED, radius, 16, wide, rout) not in (0, FS_ERR_UNSUPPORTED)
    # R = 0 rejects every candidate (the zero of the records: mantissa 0); cap 0 too
    rout["status"] = 5
    assert r.FeatureEvalDirect(T_HDR32, 4, features.FIND, radius, 16, rin, rout) == 0
    assert rout.tobytes() == np.zeros(1, features.FEATURE_OUT_HDR32).tobytes()
    one = np.zeros(1, features.REAL_HDR32)
    one["m"] = 1.0
    both(r, T_HDR32, 4, features.FIND, one, 0, rin)
    both(r, T_HDR32, 4, features.FIND, one, 16, rin)  # c = 0, R = 1: period 1 at the first step
    both(r, T_HDR32, 4, features.FIXED, one, 16, rin)  # period 0: no step, the zero record with status OK_DIRECT
    r.close()
