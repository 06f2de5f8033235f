"""The exact renderer's cycle check (fs_set_exact_cycle_check; exact.render / audit / stable_mask with prove_interior) on the GPU.
Truth for counts is GMP integer iteration (tests/_truth.py, run live): the check changes no pixel.  Truth for which samples are
proved, for the steps every sample takes and for how often a checkpoint has to be read back is the rule restated on Python integers
(tests/_cycle_model.py): the check depends on n alone, so all three are exact numbers, whatever the slices and the compaction do."""
import numpy as np
import pytest

import _cycle_model as model
import _truth
from fractalshark_amd import GPURenderer, T_F64, exact, inputs

pytestmark = pytest.mark.gpu

FS_ERR_6 = 10005
W, H, CAP = 64, 48, 20000


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _switches_off(renderer):
    yield
    assert renderer.SetExactCycleCheck(False) == 0
    assert renderer.SetExactCycleFingerprintBits(0) == 0
    assert renderer.SetExactSlice(0) == 0


def _view(w=W, h=H, cap=CAP):
    v = inputs.View("-2.2", "-1.2", "1.0", "1.2", w, h)
    v.num_iterations = cap
    return v


_models, _truths = {}, {}


def _model(v, F, R=4, inclusive=False):
    """The model over the view's whole frame, row-major, once per configuration: what the model said when
    tests/golden/make_exact_cycle_model.py ran it on these very axes where that is recorded (the 64 x 48 frames: up to a quarter of a
    minute of Python integers each), else run here."""
    key = (tuple(v.bbox()), v.width, v.height, v.num_iterations, F, R, inclusive)
    if key not in _models:
        cx, cy = exact.axes(v, F)
        cap = v.num_iterations
        rec = model.recorded(model.record_key(v.width, v.height, F, R, inclusive, cap), model.axes_crc(cx, cy), cap)
        _models[key] = rec or model.frame(model.from_limbs(cx), model.from_limbs(cy), F, R, inclusive, cap)
    return _models[key]


def _truth_frame(v, F, R=4, inclusive=False):
    """min(E - 1, N) of every pixel from GMP integer iteration, limit = cap + 1."""
    key = (tuple(v.bbox()), v.width, v.height, v.num_iterations, F, R, inclusive)
    if key not in _truths:
        w, h, cap = v.width, v.height, v.num_iterations
        gx, gy = np.meshgrid(np.arange(w), np.arange(h))
        E, _ = _truth.exact_counts(v.bbox(), w, h, gx.ravel(), gy.ravel(), cap + 1, R, F, shifts=[], inclusive=inclusive)
        _truths[key] = _truth.expect_minus_one(E, cap).reshape(h, w)
    return _truths[key]


def _render(r, v, F, R=4, inclusive=False, iter_bytes=4, prove=False):
    """(frame, proved mask or None, exact_stats, exact_cycle_stats) of one exact.render."""
    w, h = v.width, v.height
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False, iter_bytes=iter_bytes) == 0
    assert r.ClearMemory() == 0
    mask = exact.render(r, v, bailout=R, frac_bits=F, iter_bytes=iter_bytes, inclusive=inclusive, prove_interior=prove)
    st, cst = r.exact_stats(), r.exact_cycle_stats()
    out = r.new_iter_buffer()
    assert r.RenderCurrent(v.num_iterations, out) == 0 and r.SyncComputeStream() == 0
    return out[:h, :w].copy(), mask, st, cst


def _check_on(v, m, got, what):
    """One check-on render against the model: mask, step total and proof count."""
    frame, mask, st, cst = got
    h, w = frame.shape
    print("cycle %-34s proved %d (model %d), steps %d (model %d), compares %d (model %d / %d / %d at 64 / 4 / 1 bits), launches %d" % (
        what, int(mask.sum()), int(m.proved.sum()), st["lane_steps"], int(m.steps.sum()), cst[1], m.hit_totals[2], m.hit_totals[1],
        m.hit_totals[0], st["launches"]))
    assert mask.dtype == bool and mask.shape == (h, w)
    assert np.array_equal(mask, m.proved.reshape(h, w)), int((mask != m.proved.reshape(h, w)).sum())
    assert st["lane_steps"] == int(m.steps.sum())
    assert cst[0] == int(mask.sum())


@pytest.mark.parametrize("F,R,inclusive,iter_bytes", [(54, 4, False, 4), (246, 4, False, 4), (758, 4, False, 4), (246, 256, False, 4),
                                                      (246, 4, True, 4), (246, 4, False, 8)])
def test_frame_mask_and_steps(renderer, F, R, inclusive, iter_bytes):
    assert exact.limbs_for(F) == {54: 2, 246: 8, 758: 24}[F]
    v = _view()
    m, want = _model(v, F, R, inclusive), _truth_frame(v, F, R, inclusive)
    n_esc, n_proved, n_capped = m.kinds()
    assert n_esc > 0 and n_proved > 0 and n_capped > 0
    assert np.array_equal(m.value.reshape(H, W), want)  # (the model agrees with GMP before it judges anything else)
    on = _render(renderer, v, F, R, inclusive, iter_bytes, prove=True)
    _check_on(v, m, on, "F %d R %d incl %d ib %d" % (F, R, inclusive, iter_bytes))
    assert int((on[0].astype(np.int64) != want).sum()) == 0
    assert on[3][1] == m.hit_totals[2]  # the full fingerprint: the model's 64-bit matches
    off_frame, off_mask, off_st, off_cst = _render(renderer, v, F, R, inclusive, iter_bytes)
    assert off_mask is None and off_cst == (0, 0) and renderer.ExactProved()[0] == FS_ERR_6
    assert off_frame.dtype == on[0].dtype == (np.uint64 if iter_bytes == 8 else np.uint32)
    assert off_frame.tobytes() == on[0].tobytes()
    assert off_st["lane_steps"] == int(m.steps_off.sum())
    # A check that never fires cannot pass: at 54 and 246 fractional bits the model cuts the steps by factors of 12 and 6.1, and
    # the bar is 4.  At 758 it is 3: a proof lands after about F / log2(1 / |lambda|) periods, so with three times the fractional
    # bits of 246 and the same cap the proofs come three times later (537 proved, 3 968 842 steps against 12 179 191: 3.07).
    assert on[2]["lane_steps"] < off_st["lane_steps"] // (4 if F <= 246 else 3)


def test_carried_state(renderer):
    """The checkpoint travels with its sample from slice to slice and from slot to slot: slices of 16 steps with and without
    compaction, and of 1000 (no power of two: checkpoints are retaken inside slices and at their ends)."""
    r, F = renderer, 246
    v = _view()
    m = _model(v, F)
    base = _render(r, v, F, prove=True)
    _check_on(v, m, base, "F 246 default slices")
    for steps, loose in ((16, False), (16, True), (1000, False)):
        assert r.SetExactSlice(steps, no_compaction=loose) == 0
        got = _render(r, v, F, prove=True)
        _check_on(v, m, got, "F 246 slice %d%s" % (steps, " no compaction" if loose else ""))
        assert got[0].tobytes() == base[0].tobytes() and got[3] == base[3]
        assert got[2]["launches"] == -(-int(m.steps.max()) // steps)
    assert int(m.steps.max()) == CAP + 1  # (the capped, unproved samples: 1251 launches of 16 steps)


def test_full_compare_says_no(renderer):
    """With a fingerprint of 4 bits or 1 bit the checkpoint is read back on every 16th or every second step, and nearly every
    time the answer must be "not equal": a compare that always says yes, or reads another sample's slot, proves samples that escape."""
    r, F = renderer, 246
    v = _view()
    m = _model(v, F)
    base = _render(r, v, F, prove=True)
    for bits, col in ((4, 1), (1, 0)):
        assert r.SetExactCycleFingerprintBits(bits) == 0
        got = _render(r, v, F, prove=True)
        _check_on(v, m, got, "F 246 fingerprint of %d bits" % bits)
        assert got[0].tobytes() == base[0].tobytes()
        want = m.hit_totals[col]
        assert got[3][1] >= want > 50 * int(m.proved.sum()), (bits, got[3][1], want)
    # ... and with slices and compaction in between
    assert r.SetExactSlice(100) == 0
    got = _render(r, v, F, prove=True)
    _check_on(v, m, got, "F 246 fingerprint of 1 bit, slice 100")
    assert got[0].tobytes() == base[0].tobytes() and got[3][1] >= m.hit_totals[0]


def test_fixture_frame(renderer):
    c = _truth.Case("view0_70x37")
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    assert (v.width, v.height) == (c.w, c.h) == (70, 37)
    m = _model(v, F)
    n_esc, n_proved, n_capped = m.kinds()
    print("cycle view0_70x37: F %d cap %d, model: %d escape, %d proved, %d capped and unproved" % (F, c.cap, n_esc, n_proved, n_capped))
    assert n_proved >= 1 and n_capped >= 1
    on = _render(renderer, v, F, prove=True)
    _check_on(v, m, on, "view0_70x37")
    assert np.array_equal(c.sample(on[0]), _truth.expect_minus_one(c.counts(4), c.cap))
    off = _render(renderer, v, F)
    assert off[0].tobytes() == on[0].tobytes() and off[2]["lane_steps"] == int(m.steps_off.sum())


def _audit_runs(v, F, xs, ys, levels):
    """(cx, cy) of the audit's runs as Python integers, in run order: run 0 = c, run 1 + 4 j + d = c + s_j, c - s_j, c + i s_j, c - i s_j."""
    L = exact.limbs_for(F)
    cx, cy = exact.axes(v, F, limbs=L)
    cxs, cys = model.from_limbs(cx[:, xs]), model.from_limbs(cy[:, ys])
    for level in levels:
        cx3, cy3 = exact.axes(v, F, level=level, limbs=L)
        for ax, ay in ((cx3[1], cy3[0]), (cx3[2], cy3[0]), (cx3[0], cy3[1]), (cx3[0], cy3[2])):
            cxs += model.from_limbs(ax[:, xs])
            cys += model.from_limbs(ay[:, ys])
    return cxs, cys


def test_audit(renderer):
    """A binary64 direct frame audited on a 16 x 12 lattice at two levels, check on and off: the same report, fewer steps."""
    r = renderer
    v = _view()
    assert r.InitializeMemory(W, H, 1, None, 0, 0, 0, False) == 0 and r.ClearMemory() == 0
    dx, dy, minx, maxy = v.coords_direct_f64()
    assert r.Render(None, minx, maxy, dx, dy, CAP, T=T_F64) == 0 and r.SyncComputeStream() == 0
    xs, ys = exact.lattice(v, 16, 12)
    levels, F = (10, 20), v.precision_bits + exact.GUARD_BITS
    assert len(xs) == 192 and not exact.uses_wide(exact.limbs_for(F))
    off = exact.audit(r, v, xs, ys, levels=levels, bailout=4)
    off_steps = r.exact_stats()["lane_steps"]
    assert (off.n_proved, off.proved) == (0, None) and r.ExactProved(9 * 192)[0] == FS_ERR_6
    on = exact.audit(r, v, xs, ys, levels=levels, bailout=4, prove_interior=True)
    on_steps, cst = r.exact_stats()["lane_steps"], r.exact_cycle_stats()
    err, proved_runs = r.ExactProved(9 * 192)
    assert err == 0
    assert bytes(on.record) == bytes(off.record) and on.as_dict() == off.as_dict() and on.offenders == off.offenders
    assert np.array_equal(on.values, off.values) and np.array_equal(on.frame_values, off.frame_values)
    assert np.array_equal(on.stable, off.stable)
    m = model.Runs(*_audit_runs(v, F, xs.astype(np.int64), ys.astype(np.int64), levels), F, 4, False, CAP)
    print("cycle audit: %d runs, %d proved (model %d), %d of the %d centre runs; steps %d on, %d off" % (
        len(m.steps), int(proved_runs.sum()), int(m.proved.sum()), on.n_proved, len(xs), on_steps, off_steps))
    assert np.array_equal(proved_runs.astype(bool), m.proved) and cst[0] == int(m.proved.sum()) > 0
    assert on.n_proved == int(m.proved[:192].sum()) > 0 and np.array_equal(on.proved, m.proved[:192])
    assert np.array_equal(on.values, m.value[:192])
    assert (on_steps, off_steps) == (int(m.steps.sum()), int(m.steps_off.sum())) and on_steps < off_steps


def test_stable_mask(renderer):
    r = renderer
    v = _view()
    F = v.precision_bits + exact.GUARD_BITS
    centre = _render(r, v, F, prove=True)
    want_proved = centre[1]
    off = exact.stable_mask(r, v, 12)
    off_steps = r.exact_stats()["lane_steps"]
    assert r.ExactProved()[0] == FS_ERR_6  # a call with the check off
    on = exact.stable_mask(r, v, 12, prove_interior=True)
    on_steps = r.exact_stats()["lane_steps"]
    print("cycle stable mask at 2^-12: %d of %d stable; steps %d on, %d off" % (int(on.sum()), on.size, on_steps, off_steps))
    assert on.dtype == bool and np.array_equal(on, off) and 0 < int(on.sum()) < on.size
    assert on_steps < off_steps and r.exact_cycle_stats()[0] > 0
    # the centre frame and its mask are left alone
    again = _render(r, v, F, prove=True)
    assert again[0].tobytes() == centre[0].tobytes() and np.array_equal(again[1], want_proved)
    assert np.array_equal(exact.stable_mask(r, v, 12, prove_interior=True), on)
    err, kept = r.ExactProved()
    assert err == 0 and np.array_equal(kept.reshape(H, W).astype(bool), want_proved)


def test_switch_is_off_by_default(native_libs):
    fresh = GPURenderer(0)
    try:
        v = _view(16, 12, 500)
        frame, mask, st, cst = _render(fresh, v, 54)
        assert mask is None and cst == (0, 0) and fresh.ExactProved()[0] == FS_ERR_6
        assert st["lane_steps"] == int(np.where(frame == 500, 501, frame.astype(np.int64) + 1).sum())
        on = _render(fresh, v, 54, prove=True)
        assert on[0].tobytes() == frame.tobytes() and on[1].sum() == on[3][0] > 0 and fresh.ExactProved()[0] == 0
        assert fresh.ExactProved(5)[0] == 1  # hipErrorInvalidValue: not the mask's size
        # exact.render has switched the check off again behind itself
        again = _render(fresh, v, 54)
        assert again[2] == st and again[3] == (0, 0) and fresh.ExactProved()[0] == FS_ERR_6
    finally:
        fresh.close()


def test_wide_path_ignores_the_switch(renderer):
    r = renderer
    v = _truth.boundary_view(inputs)
    n, cap, F, L = _truth.BOUNDARY_SIZE, _truth.BOUNDARY_CAP, 790, 25
    assert exact.uses_wide(L) and exact.limbs_for(F) == L
    cx, cy = exact.axes(v, F, limbs=L)
    assert r.InitializeMemory(n, n, 1, None, 0, 0, 0, False) == 0

    def wide():
        assert r.ClearMemory() == 0
        assert r.RenderExactWide(4, F, L, cx, cy, 4, False, cap) == 0
        out = r.new_iter_buffer()
        assert r.RenderCurrent(cap, out) == 0 and r.SyncComputeStream() == 0
        return out[:n, :n].copy(), r.exact_stats(), r.exact_cycle_stats(), r.ExactProved()[0]

    off = wide()
    assert r.SetExactCycleCheck(True) == 0
    on = wide()
    assert on[0].tobytes() == off[0].tobytes() and on[1:] == off[1:] and on[2] == (0, 0) and on[3] == FS_ERR_6
    assert int((on[0] == cap).sum()) > 0  # (samples the narrow path would have proved: c = 0 among them)
    assert r.SetExactCycleCheck(False) == 0
    assert exact.render(r, v, bailout=4, frac_bits=F, prove_interior=True) is None
    assert r.exact_cycle_stats() == (0, 0) and r.ExactProved()[0] == FS_ERR_6
