"""fs_exact_audit (fractalshark_amd.exact.audit) on the GPU: the exact counts and stability bits it computes against the GMP
fixture, and every number of its record against a numpy restatement (tests/_audit.py) on the read-back frame -- exact frames,
deliberately wrong frames, LAv2 frames in both mantissa widths; the narrow (one lane per run) and the wide (one wave per run)
path; slices, IterTypes, a frame in a torch tensor, error codes, frame state.  Integer equality throughout."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _audit
import _truth
from fractalshark_amd import GPURenderer, LAV2_FULL, PARITY_CPU, PARITY_CPU_GPUSTAGE, T_HDR32, T_HDR64, _capi, exact, inputs
from fractalshark_amd.renderer import FS_ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu

FS_ERR_6 = 10005
HIP_INVALID_VALUE = 1
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.SetExactSlice(0)
    r.close()


def _frame(r, n):
    out = r.new_iter_buffer()
    assert r.RenderCurrent(n, out) == 0
    assert r.SyncComputeStream() == 0
    return out


def _render_exact(r, v, w, h, R, F, cap, iter_bytes=4):
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False, iter_bytes=iter_bytes) == 0
    assert r.ClearMemory() == 0
    v.num_iterations = cap
    exact.render(r, v, bailout=R, frac_bits=F, iter_bytes=iter_bytes)
    return _frame(r, cap)


def _fixture_stable(c, R):
    return np.stack([c.stable(R, lv) for lv in c.ladder], axis=1)


def _check_report(rep, c, frame, exact_values, stable, cap):
    """Every number of the report against numpy on the read-back frame."""
    fv = c.sample(frame)
    want = _audit.expected(fv, exact_values, stable, cap)
    _audit.same_record(rep.record, want)
    assert np.array_equal(rep.values, exact_values) and np.array_equal(rep.frame_values, fv) and np.array_equal(rep.stable, stable)
    assert (rep.n_differ, rep.n_equal, rep.n_capped) == (want["n_differ"], want["n_equal"], want["n_capped"])
    assert rep.stable_count == want["stable"] and rep.stable_differ == want["stable_differ"]
    assert rep.max_abs_diff == want["max_abs_diff"] and rep.stable_capped == want["stable_capped"]
    assert [(o["sample"], o["frame_value"], o["exact_value"]) for o in rep.offenders] == [(i, f, e) for i, _, f, e in want["offenders"]]
    assert all((o["x"], o["y"]) == (c.xs[o["sample"]], c.ys[o["sample"]]) for o in rep.offenders)
    return want


@pytest.mark.parametrize("name,R", [("shallow_1e-20", 4), ("shallow_1e-20", 256), ("view0_70x37", 4), ("view3_64x36", 256)])
def test_values_and_stability_equal_the_fixture(renderer, name, R):
    c = _truth.Case(name)
    v, F = c.view(inputs), c.raw["frac_bits"]
    assert exact.limbs_for(F) == {"shallow_1e-20": 9, "view0_70x37": 7, "view3_64x36": 11}[name] and len(c.ladder) == 8
    frame = _render_exact(renderer, v, c.w, c.h, R, F, c.cap)
    rep = exact.audit(renderer, v, c.xs, c.ys, levels=c.ladder, bailout=R, frac_bits=F)
    want_values = _truth.expect_minus_one(c.counts(R), c.cap)
    bad = int((rep.values != want_values).sum())
    print("audit %-14s R%-3d %d samples x %d runs: %d values differ from the fixture, stable per level %s, %d capped, launches %d" % (
        name, R, len(c.xs), 1 + 4 * len(c.ladder), bad, rep.stable_count, rep.n_capped, renderer.exact_stats()["launches"]))
    assert bad == 0
    for j, lv in enumerate(c.ladder):
        want = c.stable(R, lv)
        assert np.array_equal(rep.stable[:, j], want), (lv, int((rep.stable[:, j] != want).sum()))
        assert rep.stable_count[j] == int(want.sum())
    assert rep.n_differ == 0 and rep.n_equal == len(c.xs) and rep.offenders == [] and rep.stable_differ == [0] * 8
    assert rep.max_abs_diff == [0] * 8
    assert rep.n_capped == int((want_values == c.cap).sum())
    _check_report(rep, c, frame, want_values, _fixture_stable(c, R), c.cap)


def test_a_wrong_frame_is_reported_exactly(renderer):
    c = _truth.Case("shallow_1e-20")
    v, F = c.view(inputs), c.raw["frac_bits"]
    want_values, stable = _truth.expect_minus_one(c.counts(256), c.cap), _fixture_stable(c, 256)
    # what the fixture guarantees: no capped sample at R 256, counts beyond cap // 4, and R 4 counts that differ from R 256's
    assert not (c.counts(256) == 0).any() and (want_values > c.cap // 4).any() and (c.counts(4) != c.counts(256)).any()
    # a frame cut off at a quarter of the cap, audited at the full cap
    frame = _render_exact(renderer, v, c.w, c.h, 256, F, c.cap // 4)
    v.num_iterations = c.cap
    rep = exact.audit(renderer, v, c.xs, c.ys, levels=c.ladder, bailout=256, frac_bits=F)
    want = _check_report(rep, c, frame, want_values, stable, c.cap)
    print("audit wrong frame (cap / 4): %d of %d differ, stable_differ %s, max_abs_diff %s" % (
        rep.n_differ, rep.n_samples, rep.stable_differ, rep.max_abs_diff))
    assert rep.n_differ > 0 and rep.n_offenders == min(16, rep.n_differ) == len(want["offenders"])
    # the R 4 frame audited at R 256
    frame = _render_exact(renderer, v, c.w, c.h, 4, F, c.cap)
    rep = exact.audit(renderer, v, c.xs, c.ys, levels=c.ladder, bailout=256, frac_bits=F)
    _check_report(rep, c, frame, want_values, stable, c.cap)
    print("audit wrong frame (R 4 at R 256): %d of %d differ, stable_differ %s, max_abs_diff %s" % (
        rep.n_differ, rep.n_samples, rep.stable_differ, rep.max_abs_diff))
    assert rep.n_differ > 0


@pytest.mark.parametrize("is64", [False, True])
def test_a_real_kernel(renderer, is64):
    """LAv2 Full in the GPU's stage-test direction: the audit's per-level numbers are numpy's, the level the fixture chose for the
    width is clean, and finest_clean_level() finds a level at least as fine."""
    r = renderer
    c = _truth.Case("shallow_1e-20")
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    ob = inputs.Orbit(v, is64=is64)
    la = inputs.LATable(ob)
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0
    assert r.InitializePerturb(1, ob, 0, None, la) == 0
    assert r.ClearMemory() == 0
    co = [(float(t["m"]), int(t["e"])) for t in v.coords_perturb(ob)]
    assert r.RenderPerturbLAv2(None, None, None, *co, c.cap, T=T_HDR64 if is64 else T_HDR32, Mode=LAV2_FULL,
                               parity=PARITY_CPU_GPUSTAGE) == 0
    assert r.SyncComputeStream() == 0
    frame = _frame(r, c.cap)
    rep = exact.audit(r, v, c.xs, c.ys, levels=c.ladder, bailout=256, frac_bits=F)
    _check_report(rep, c, frame, _truth.expect_minus_one(c.counts(256), c.cap), _fixture_stable(c, 256), c.cap)
    key = ("m53" if is64 else "m24") + "_lav2_gpustage"
    level = c.levels[key]["level"]
    finest = rep.finest_clean_level()
    print("audit lav2 full %s: stable %s, stable_differ %s, fixture level 2^-%d, finest clean level %s" % (
        key, rep.stable_count, rep.stable_differ, level, finest))
    assert _truth.carries(c.name, key)
    assert rep.stable_differ[c.ladder.index(level)] == 0
    assert finest is not None and finest >= level


def test_wide_path_and_narrow_wide_agreement(renderer):
    r = renderer
    c = _truth.Case("shallow_1e-6")
    w, h, cap, levels = 16, 9, 20000, (17, 25)
    b = c.raw["bbox"]
    v = inputs.View(b[0], b[1], b[2], b[3], w, h, num_iterations=cap)
    xs, ys = exact.lattice(v, w, h)
    assert len(xs) == w * h
    got = {}
    for F in (204, 759):
        assert exact.uses_wide(exact.limbs_for(F)) == (F == 759) and exact.limbs_for(759) == 25
        _render_exact(r, v, w, h, 256, F, cap)
        rep = exact.audit(r, v, xs, ys, levels=levels, bailout=256, frac_bits=F)
        values, stable = exact.sample_counts(r, v, xs, ys, bailout=256, frac_bits=F, levels=levels)
        assert np.array_equal(rep.values, values) and np.array_equal(rep.stable, stable)
        assert rep.n_differ == 0 and rep.stable_count == [int(stable[:, j].sum()) for j in range(2)]
        got[F] = rep
    assert np.array_equal(got[204].values, got[759].values) and int((got[204].values < cap).sum()) > w * h // 2


def test_slices_and_itertype(renderer):
    r = renderer
    c = _truth.Case("shallow_1e-20")
    v, F = c.view(inputs), c.raw["frac_bits"]
    records = []
    try:
        for slice_steps, iter_bytes in ((0, 4), (16, 4), (0, 8)):
            _render_exact(r, v, c.w, c.h, 4, F, c.cap, iter_bytes=iter_bytes)  # the R 4 frame: a record with something in it
            assert r.SetExactSlice(slice_steps) == 0
            rep = exact.audit(r, v, c.xs, c.ys, levels=c.ladder, bailout=256, frac_bits=F)
            assert r.SetExactSlice(0) == 0
            st = r.exact_stats()
            assert st["lane_steps"] <= st["lane_slots"] and st["lane_steps"] > 0
            if slice_steps:
                assert st["launches"] > 1
            records.append((bytes(rep.record), st["lane_steps"]))
    finally:
        r.SetExactSlice(0)
        assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False, iter_bytes=4) == 0
    assert records[0] == records[1] == records[2]
    assert exact.audit(r, v, c.xs[:0], c.ys[:0], levels=c.ladder, bailout=256, frac_bits=F).n_samples == 0


def test_device_iters_in_a_torch_tensor(native_libs):
    """The frame handed over in a torch device tensor: torch has to bring the GPU up before the library does, so this runs in a
    fresh child process (tests/exact/torch_audit.py)."""
    p = subprocess.run([sys.executable, os.path.join(HERE, "exact", "torch_audit.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULTS ")][-1]
    assert json.loads(line[len("RESULTS "):]) == {"device_iters": "ok"}


def _limbs_of(value, limbs):
    return [(value >> (32 * l)) & 0xFFFFFFFF for l in range(limbs)]


def test_error_returns(renderer):
    F, L, n = 187, 7, 5
    xs, ys = np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)
    cxr, cyr = np.zeros((5, L, n), np.uint32), np.zeros((5, L, n), np.uint32)
    res = _capi.AuditResult()
    p = lambda a: None if a is None else a.ctypes.data

    def call(r, F=F, L=L, xs=xs, ys=ys, n=n, k=1, cx=cxr, cy=cyr, R=256, cap=100, out=res):
        return r._lib.fs_exact_audit(r._h, None, F, L, p(xs), p(ys), n, k, p(cx), p(cy), R, 0, cap,
                                     C.byref(out) if out is not None else None, None, None, None)

    fresh = GPURenderer(0)
    try:
        assert call(fresh) == FS_ERR_6
    finally:
        fresh.close()
    r = renderer
    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False) == 0 and r.ClearMemory() == 0
    assert call(r) == 0 and (res.n_samples, res.n_levels, res.n_equal) == (n, 1, 0)  # c = 0 never escapes: 100, the frame holds 0
    assert call(r, L=1, F=10) == FS_ERR_UNSUPPORTED and call(r, L=705) == FS_ERR_UNSUPPORTED
    assert call(r, L=6) == FS_ERR_UNSUPPORTED                                     # 32 * 6 < 187 + 10
    assert call(r, R=0) == FS_ERR_UNSUPPORTED and call(r, R=257) == FS_ERR_UNSUPPORTED and call(r, R=1) == 0
    assert call(r, k=9) == FS_ERR_UNSUPPORTED
    for name in ("xs", "ys", "cx", "cy", "out"):
        assert call(r, **{name: None}) == HIP_INVALID_VALUE, name
    assert call(r, xs=np.array([0, 1, 64, 3, 4], np.uint32)) == HIP_INVALID_VALUE  # a sample outside the frame
    assert call(r, ys=np.array([0, 1, 2, 36, 4], np.uint32)) == HIP_INVALID_VALUE
    assert call(r, xs=np.array([0, 1, 63, 3, 4], np.uint32), ys=np.array([0, 1, 2, 35, 4], np.uint32)) == 0
    assert call(r, n=0x7FFFFFFF // 33 + 1, k=8) == HIP_INVALID_VALUE               # more than 2^31 - 1 runs (refused before any array is read)
    assert call(r, cap=1 << 32) == HIP_INVALID_VALUE and call(r, cap=(1 << 64) - 1) == HIP_INVALID_VALUE
    far = cxr.copy()
    far[3, :, 2] = _limbs_of(32 << F, L)                                          # c = 32 in one run
    assert call(r, cx=far) == FS_ERR_UNSUPPORTED and call(r, cy=far) == FS_ERR_UNSUPPORTED
    # two faults at once: the first refusal in the header's order decides
    assert call(r, k=9, out=None) == FS_ERR_UNSUPPORTED                            # the levels before a NULL record
    assert call(r, n=0, out=None) == HIP_INVALID_VALUE                             # a NULL record before "no samples"
    assert call(r, xs=np.array([0, 1, 64, 3, 4], np.uint32), cx=far) == HIP_INVALID_VALUE  # a sample outside the frame before the axis range
    assert call(r, L=6, cap=1 << 32) == FS_ERR_UNSUPPORTED                         # the format before the cap
    far[3, :, 2] = _limbs_of(-32 << F, L)                                         # c = -32 is inside
    assert call(r, cx=far) == 0
    res.n_samples = 77
    assert call(r, n=0) == 0 and bytes(res) == bytes(C.sizeof(res))                # no samples: a zeroed record
    res.n_samples = 77
    assert call(r, n=0, xs=None) == 0 and bytes(res) == bytes(C.sizeof(res))       # ... before the NULL arrays
    assert r.SetRowBands(0, 8, 16) == 0
    try:
        assert call(r) == FS_ERR_UNSUPPORTED
    finally:
        assert r.SetRowBands(0, 0, 0) == 0
    # a cap beyond 32 bits is accepted with a uint64 frame (every run at c = 31: |z_1|^2 > 256, so no run takes a second step)
    out = cxr.copy()
    out[:, :, :] = np.array(_limbs_of(31 << F, L), np.uint32)[None, :, None]
    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False, iter_bytes=8) == 0
    try:
        assert r.ClearMemory() == 0
        assert call(r, cap=1 << 32, cx=out) == 0 and (res.n_equal, res.n_capped, list(res.stable[:1])) == (n, 0, [n])
    finally:
        assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False, iter_bytes=4) == 0


def test_frame_state_is_left_as_it_was(renderer):
    """An orbit and an LA table resident before an audit render the same LAv2 frame after it; the frame, the kernel-time history
    and the tile-cost record are untouched."""
    r = renderer
    v = inputs.View.builtin(5, 64, 36)
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False) == 0
    assert r.InitializePerturb(7, ob, 0, None, la) == 0
    co = [(float(c["m"]), int(c["e"])) for c in v.coords_perturb_hdr32(ob)]
    lav2 = lambda: r.RenderPerturbLAv2(None, None, None, *co, v.num_iterations, T=T_HDR32, Mode=LAV2_FULL, parity=PARITY_CPU)
    assert lav2() == 0
    before = _frame(r, v.num_iterations).copy()
    ms, history, costs = r.last_kernel_ms(), r.kernel_ms_history(1), r.read_tile_costs()
    assert ms > 0
    xs, ys = exact.lattice(v, 8, 6)
    n_view, v.num_iterations = v.num_iterations, 2000  # (a short cap: this test is about state, not counts)
    rep = exact.audit(r, v, xs, ys, levels=(17, 30), bailout=256)
    v.num_iterations = n_view
    assert rep.n_samples == 48 and np.array_equal(rep.frame_values, before[ys, xs].astype(np.int64))
    assert r.last_kernel_ms() == ms and r.kernel_ms_history(1) == history
    after_costs = r.read_tile_costs()
    assert (costs is None and after_costs is None) or np.array_equal(costs, after_costs)
    assert _frame(r, v.num_iterations).tobytes() == before.tobytes()
    assert lav2() == 0
    assert _frame(r, v.num_iterations).tobytes() == before.tobytes()
