"""The exact renderer's continuation (fs_set_exact_keep, fs_render_exact_continue, fs_exact_kept_info, fs_exact_drop_kept; exact.render
with keep, exact.continue_render, exact.render_progressive) on the GPU.  The contract is the renderer's own: after a continuation to
the cap N the iteration buffer is, byte for byte, what a fresh call with that cap writes on the same renderer, which at the last cap
of a chain is also compared with GMP integer iteration (tests/_truth.py, run live).  The work condition

    0 <= steps(first call) + steps(continuations) - steps(fresh call at the cap) <= samples kept by the calls before

is what keeps "start over internally" from passing: the slack is the one escape test a resumed sample of the wide path repeats (the
lane path repeats nothing, its difference is zero)."""
import numpy as np
import pytest

import _truth
from fractalshark_amd import GPURenderer, LAV2_FULL, PARITY_CPU, T_F64, T_HDR32, autozoom, exact, inputs

pytestmark = pytest.mark.gpu

FS_ERR_6 = 10005
INVALID = 1  # hipErrorInvalidValue
W, H = 64, 48
BBOX = ("-2.2", "-1.2", "1.0", "1.2")
CAPS = (1022, 2500, 5000)  # 1022 + 2 is a power of two: the resumed samples retake their checkpoint in the deferred check
FS = {2: 54, 8: 246, 24: 758}


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
    assert renderer.SetExactSlice(0) == 0
    assert renderer.SetExactKeep(False) == 0
    assert renderer.DropExactKept() == 0


def _view(w=W, h=H, bbox=BBOX):
    return inputs.View(*bbox, w, h)


def _init(r, w, h, iter_bytes=4):
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False, iter_bytes=iter_bytes) == 0
    assert r.ClearMemory() == 0


def _frame(r, w, h, cap):
    out = r.new_iter_buffer()
    assert r.RenderCurrent(cap, out) == 0 and r.SyncComputeStream() == 0
    return out[:h, :w].copy()


class Stage:
    """What one exact call left: the frame, the proved mask (None with the check off) and its statistics.  check = None: the
    mask is the caller's to read."""

    def __init__(self, r, w, h, cap, check=None):
        self.frame = _frame(r, w, h, cap)
        self.stats, self.cycle = r.exact_stats(), r.exact_cycle_stats()
        self.steps = self.stats["lane_steps"]
        self.mask = None
        if check is not None:
            err, mask = r.ExactProved()
            assert err == (0 if check else FS_ERR_6)
            self.mask = mask.reshape(h, w).astype(bool) if check else None


_axes, _fresh, _truths = {}, {}, {}


def _axes_of(w, h, F, L):
    if (w, h, F, L) not in _axes:
        _axes[(w, h, F, L)] = exact.axes(_view(w, h), F, limbs=L)
    return _axes[(w, h, F, L)]


def _call(r, wide, ib, F, L, cx, cy, R, inclusive, cap):
    return (r.RenderExactWide if wide else r.RenderExact)(ib, F, L, cx, cy, R, inclusive, cap)


def _fresh_stage(r, w, h, F, L, R, inclusive, ib, check, wide, cap):
    """A fresh call at the cap with keep off, once per configuration (the renderer must hold the w x h frame of ib bytes)."""
    key = (w, h, F, L, R, inclusive, ib, check, wide, cap)
    if key not in _fresh:
        cx, cy = _axes_of(w, h, F, L)
        assert r.SetExactKeep(False) == 0 and r.SetExactCycleCheck(check) == 0
        assert r.SetExactSlice(0) == 0
        assert _call(r, wide, ib, F, L, cx, cy, R, inclusive, cap) == 0
        _fresh[key] = Stage(r, w, h, cap, check and not wide)
        assert r.ExactKept()["valid"] == 0  # keep off leaves nothing
    return _fresh[key]


def _truth_frame(w, h, F, R, inclusive, cap):
    key = (w, h, F, R, inclusive, cap)
    if key not in _truths:
        gx, gy = np.meshgrid(np.arange(w), np.arange(h))
        # (the view's own reading of the bounding box, as exact.axes takes it)
        E, _ = _truth.exact_counts(_view(w, h).bbox(), w, h, gx.ravel(), gy.ravel(), cap + 1, R, F, shifts=[], inclusive=inclusive)
        _truths[key] = _truth.expect_minus_one(E, cap).reshape(h, w)
    return _truths[key]


def _chain(r, L, F, caps, R=256, inclusive=False, ib=4, check=False, wide=False, w=W, h=H, slice_steps=0, no_compaction=False,
           truth=True):
    """keep at caps[0], continue through the rest: every stage against the fresh call at its cap."""
    _init(r, w, h, ib)
    check_runs = check and not wide
    fresh = [_fresh_stage(r, w, h, F, L, R, inclusive, ib, check, wide, cap) for cap in caps]
    _fresh_stage(r, w, h, F, L, R, inclusive, ib, check, wide, caps[-1] + 1)  # (read below; rendered before anything is kept)
    cx, cy = _axes_of(w, h, F, L)
    assert r.SetExactSlice(slice_steps, no_compaction) == 0
    assert r.SetExactKeep(True) == 0 and r.SetExactCycleCheck(check) == 0
    steps = proofs = kept_before = 0
    for k, cap in enumerate(caps):
        if k == 0:
            assert _call(r, wide, ib, F, L, cx, cy, R, inclusive, cap) == 0
            # the switches recorded with the set are what a continuation uses, not the current ones
            assert r.SetExactCycleCheck(not check) == 0
        else:
            assert r.RenderExactContinue(cap) == 0
        if k == 1:
            assert r.SetExactCycleCheck(check) == 0  # (ExactProved reads the last call's mask either way)
        st = Stage(r, w, h, cap)
        f = fresh[k]
        assert st.frame.dtype == (np.uint64 if ib == 8 else np.uint32)
        assert st.frame.tobytes() == f.frame.tobytes(), (k, cap, int((st.frame != f.frame).sum()))
        err, mask = r.ExactProved()
        if check_runs:
            assert err == 0 and np.array_equal(mask.reshape(h, w).astype(bool), f.mask), (k, cap)
        else:
            assert err == FS_ERR_6
        steps += st.stats["lane_steps"]
        proofs += st.cycle[0]
        slack = steps - f.steps
        print("keep L %d F %d R %d incl %d ib %d check %d wide %d slice %d/%d cap %d: steps %d (chain) %d (fresh), slack %d <= %d, "
              "launches %d" % (L, F, R, inclusive, ib, check, wide, slice_steps, no_compaction, cap, steps, f.steps, slack, kept_before,
                               st.stats["launches"]))
        assert 0 <= slack <= kept_before, (k, cap, slack, kept_before)
        # the lane path repeats nothing; every resumed sample of the wide path repeats exactly its one escape test
        assert slack == (kept_before if wide else 0)
        if check_runs:
            assert proofs == f.cycle[0] == int(f.mask.sum())
        info = r.ExactKept()
        # kept: neither escaped by n = cap + 1 (such a sample holds more than the cap under any larger one) nor proved
        beyond = fresh[k + 1] if k + 1 < len(caps) else _fresh_stage(r, w, h, F, L, R, inclusive, ib, check, wide, cap + 1)
        unproved = beyond.frame.astype(np.int64) > cap
        if check_runs:
            unproved &= ~f.mask
        assert info["valid"] == 1 and info["cap"] == cap and info["device_bytes"] > 0
        assert info["samples"] == int(unproved.sum()) and info["proved"] == (int(f.mask.sum()) if check_runs else 0)
        assert (info["frac_bits"], info["limbs"], info["bailout"], info["inclusive"]) == (F, L, R, int(inclusive))
        assert (info["wide"], info["cycle_check"]) == (int(wide), int(check_runs))
        assert info["device_bytes"] < 256 + 4096 + (info["samples"] + 64) * (16 * L + 12) + w * h + 8 * L * (w + h)  # not W x H states
        kept_before += info["samples"]
    assert kept_before > 0  # (the frame has an interior: something was resumed)
    if truth:
        want = _truth_frame(w, h, F, R, inclusive, caps[-1])
        assert int((st.frame.astype(np.int64) != want).sum()) == 0
    return st


@pytest.mark.parametrize("check", [False, True])
@pytest.mark.parametrize("L", [2, 8, 24])
def test_lane_chain(renderer, L, check):
    _chain(renderer, L, FS[L], CAPS, check=check)


@pytest.mark.parametrize("check", [False, True])
@pytest.mark.parametrize("slice_steps,no_compaction", [(16, False), (16, True), (1000, False), (1000, True)])
def test_lane_chain_slices(renderer, slice_steps, no_compaction, check):
    """Slices of 16 steps with and without compaction, and of 1000, which divides none of the caps' step counts."""
    assert all((cap + 1) % 1000 for cap in CAPS)
    _chain(renderer, 8, FS[8], CAPS, check=check, slice_steps=slice_steps, no_compaction=no_compaction, truth=False)


@pytest.mark.parametrize("R,inclusive,ib", [(256, False, 8), (256, True, 4), (4, False, 4), (4, True, 8)])
def test_lane_chain_formats(renderer, R, inclusive, ib):
    try:
        _chain(renderer, 8, FS[8], CAPS, R=R, inclusive=inclusive, ib=ib, check=True)
        _chain(renderer, 8, FS[8], CAPS, R=R, inclusive=inclusive, ib=ib, check=False, truth=False)
    finally:
        _init(renderer, W, H, 4)


@pytest.mark.parametrize("L", [25, 130])
def test_wide_chain(renderer, L):
    """One limb per lane and several: the view at 16 x 12, caps 50 -> 300."""
    _chain(renderer, L, 32 * L - 10, (50, 300), wide=True, w=16, h=12)


def test_wide_keep_equals_lane_fresh(renderer):
    """At 24 limbs both paths accept the call: the wide path kept at 50 and continued to 300 is the lane path's fresh frame."""
    r, L, F, w, h = renderer, 24, FS[24], 16, 12
    _init(r, w, h)
    lane = _fresh_stage(r, w, h, F, L, 256, False, 4, False, False, 300)
    st = _chain(r, L, F, (50, 300), wide=True, w=w, h=h)
    assert st.frame.tobytes() == lane.frame.tobytes()


def test_invalidation_and_errors(renderer):
    r, L, F = renderer, 2, FS[2]
    _init(r, W, H)
    cx, cy = _axes_of(W, H, F, L)
    zero = dict.fromkeys(("samples", "proved", "cap", "device_bytes", "frac_bits", "limbs", "bailout", "inclusive", "wide",
                          "cycle_check", "valid"), 0)
    keep = lambda cap=100: r.RenderExact(4, F, L, cx, cy, 4, False, cap)
    assert r.ExactKept() == zero and r.RenderExactContinue(200) == FS_ERR_6         # before any kept render
    assert keep() == 0 and r.ExactKept() == zero and r.RenderExactContinue(200) == FS_ERR_6  # keep off
    assert r.SetExactKeep(True) == 0
    for spoil in (r.ClearMemory, lambda: r.InitializeMemory(W, H, 1, None, 0, 0, 0, True),
                  lambda: r.InitializeMemory(W, H, 1, None, 0, 0, 0, False),
                  lambda: r.Render(0, -2.2, 1.2, 3.2 / W, 2.4 / H, 100, T=T_F64), r.DropExactKept,
                  lambda: r.SetExactKeep(False) or keep()):
        assert r.SetExactKeep(True) == 0
        assert keep() == 0 and r.ExactKept()["valid"] == 1 and r.ExactKept()["samples"] > 0
        assert spoil() == 0
        assert r.ExactKept() == zero and r.RenderExactContinue(200) == FS_ERR_6
    assert r.SetExactKeep(True) == 0
    # the calls that only read the frame leave the set alone
    assert keep() == 0
    before = r.ExactKept()
    _frame(r, W, H, 100)
    assert r.ExactKept() == before and before["cap"] == 100
    # the return codes
    fresh100 = _frame(r, W, H, 100)
    assert r.RenderExactContinue(100) == 0 and r.ExactKept() == before                # N2 == N1: nothing changes
    assert _frame(r, W, H, 100).tobytes() == fresh100.tobytes()
    assert r.RenderExactContinue(99) == INVALID and r.RenderExactContinue(2 ** 64 - 1) == INVALID
    assert r.RenderExactContinue(2 ** 32) == INVALID                                  # a 4-byte frame cannot hold it
    assert r.ExactKept() == before                                                    # (a refused call leaves the set)
    assert r.RenderExactContinue(101) == 0 and r.ExactKept()["cap"] == 101
    # the kept set is no idle memory
    GPURenderer.release_idle_device_memory(0)
    assert r.ExactKept()["valid"] == 1 and r.RenderExactContinue(300) == 0
    assert r.SetExactKeep(False) == 0
    assert keep(300) == 0
    want = _frame(r, W, H, 300)
    assert r.SetExactKeep(True) == 0 and keep(100) == 0 and r.RenderExactContinue(300) == 0
    assert _frame(r, W, H, 300).tobytes() == want.tobytes()


def test_every_pixel_escapes(renderer):
    """A frame far outside the set: nothing is kept and nothing proved, and a continuation launches nothing."""
    r, L, F, w, h = renderer, 2, FS[2], 16, 12
    _init(r, w, h)
    cx, cy = exact.axes(inputs.View("3.0", "3.0", "4.0", "4.0", w, h), F, limbs=L)
    for check in (False, True):
        assert r.SetExactKeep(True) == 0 and r.SetExactCycleCheck(check) == 0
        assert r.RenderExact(4, F, L, cx, cy, 4, False, 100) == 0
        info = r.ExactKept()
        assert (info["valid"], info["samples"], info["proved"], info["cap"]) == (1, 0, 0, 100)
        before = _frame(r, w, h, 100)
        assert int(before.max()) == 0
        assert r.RenderExactContinue(5000) == 0
        assert r.exact_stats()["launches"] == 0 and r.exact_stats()["lane_steps"] == 0
        assert r.ExactKept()["cap"] == 5000 and r.ExactKept()["samples"] == 0
        assert _frame(r, w, h, 5000).tobytes() == before.tobytes()
        # the mask a fresh call at the new cap gives: all zero with the check, none without
        err, mask = r.ExactProved()
        assert (err == 0 and not mask.any() and mask.shape == (w * h,)) if check else err == FS_ERR_6
        assert r.SetExactKeep(False) == 0 and r.RenderExact(4, F, L, cx, cy, 4, False, 5000) == 0
        err2, mask2 = r.ExactProved()
        assert err2 == err and np.array_equal(mask2, mask)
    # the Python layer on the same view: every stage yields render's frame and mask
    v = inputs.View("3.0", "3.0", "4.0", "4.0", w, h)
    assert r.SetExactCycleCheck(False) == 0  # (the loop above left it on; prove_interior switches it per call)
    for prove in (False, True):
        got = list(exact.render_progressive(r, v, (100, 1000, 5000), bailout=4, frac_bits=F, prove_interior=prove))
        assert [cap for cap, _ in got] == [100, 1000, 5000]
        for cap, mask in got:
            assert (mask.dtype == bool and mask.shape == (h, w) and not mask.any()) if prove else mask is None
        assert _frame(r, w, h, 5000).tobytes() == before.tobytes()


def test_every_capped_pixel_proved(renderer):
    """A 2 x 1 frame of c = -1 and c = 0: both proved within three steps, nothing kept.  A continuation launches no slice, rewrites
    the proved pixels to the new cap and leaves the fresh call's mask."""
    r, L, F, w, h = renderer, 2, FS[2], 2, 1
    _init(r, w, h)
    cx, cy = exact.axes(inputs.View("-1.0", "-1.0", "1.0", "0.0", w, h), F, limbs=L)
    assert r.SetExactKeep(True) == 0 and r.SetExactCycleCheck(True) == 0
    assert r.RenderExact(4, F, L, cx, cy, 4, False, 100) == 0
    info = r.ExactKept()
    assert (info["valid"], info["samples"], info["proved"], info["cap"], info["cycle_check"]) == (1, 0, 2, 100, 1)
    assert _frame(r, w, h, 100).tolist() == [[100, 100]]
    assert r.RenderExactContinue(5000) == 0
    assert r.exact_stats()["launches"] == 0 and r.exact_cycle_stats() == (0, 0)
    assert _frame(r, w, h, 5000).tolist() == [[5000, 5000]]
    err, mask = r.ExactProved()
    assert err == 0 and mask.tolist() == [1, 1]
    info = r.ExactKept()
    assert (info["samples"], info["proved"], info["cap"]) == (0, 2, 5000)
    assert r.RenderExactContinue(6000) == 0 and _frame(r, w, h, 6000).tolist() == [[6000, 6000]]


def test_frame_state_is_left_as_it_was(renderer):
    """An orbit and an LA table resident: a kept render, RenderCurrent, an audit on a 4 x 3 lattice, an autozoom pick and a
    continuation give the fresh frame, and leave the orbit's memory, the kernel-time history and the tile-cost record alone."""
    r = renderer
    v = inputs.View.builtin(5, 64, 36)
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False) == 0
    assert r.InitializePerturb(11, ob, 0, None, la) == 0
    co = [(float(c["m"]), int(c["e"])) for c in v.coords_perturb_hdr32(ob)]
    lav2 = lambda: r.RenderPerturbLAv2(None, None, None, *co, v.num_iterations, T=T_HDR32, Mode=LAV2_FULL, parity=PARITY_CPU)
    assert lav2() == 0
    lav2_frame = _frame(r, 64, 36, v.num_iterations)
    ms, history, costs, orbit_bytes = r.last_kernel_ms(), r.kernel_ms_history(1), r.read_tile_costs(), r.orbit_device_bytes
    assert ms > 0 and orbit_bytes > 0
    n_view = v.num_iterations
    try:
        v.num_iterations = 600
        exact.render(r, v, bailout=256)
        fresh = _frame(r, 64, 36, 600)
        v.num_iterations = 150
        exact.render(r, v, bailout=256, keep=True)
        kept = r.ExactKept()
        assert kept["valid"] == 1 and kept["samples"] > 0 and kept["cap"] == 150
        at150 = _frame(r, 64, 36, 150)
        xs, ys = exact.lattice(v, 4, 3)
        rep = exact.audit(r, v, xs, ys, levels=(17,), bailout=256)
        assert rep.n_samples == 12 and rep.n_differ == 0
        err, res = r.AutozoomPick(autozoom.MAX, 150)
        assert err == 0
        assert r.ExactKept() == kept
        assert _frame(r, 64, 36, 150).tobytes() == at150.tobytes()
        exact.continue_render(r, 600)
        assert _frame(r, 64, 36, 600).tobytes() == fresh.tobytes()
    finally:
        v.num_iterations = n_view
    assert r.last_kernel_ms() == ms and r.kernel_ms_history(1) == history and r.orbit_device_bytes == orbit_bytes
    after_costs = r.read_tile_costs()
    assert (costs is None and after_costs is None) or np.array_equal(costs, after_costs)
    assert lav2() == 0                                            # ... which replaces the frame, and drops the set
    assert _frame(r, 64, 36, v.num_iterations).tobytes() == lav2_frame.tobytes()
    assert r.ExactKept()["valid"] == 0 and r.RenderExactContinue(1000) == FS_ERR_6


def test_python_layer(renderer):
    r, F = renderer, FS[8]
    v = _view()
    _init(r, W, H)
    caps = (200, 1000, 4000)
    want = {}
    for cap in caps:
        v.num_iterations = cap
        mask = exact.render(r, v, bailout=256, frac_bits=F, prove_interior=True)
        assert r.ExactKept()["valid"] == 0                        # keep=False, the default, leaves nothing kept
        want[cap] = (_frame(r, W, H, cap), mask)
    v.num_iterations = 7  # (the caps are render_progressive's, not the view's)
    seen = []
    for cap, mask in exact.render_progressive(r, v, reversed(caps), bailout=256, frac_bits=F, prove_interior=True):
        seen.append(cap)
        assert _frame(r, W, H, cap).tobytes() == want[cap][0].tobytes()
        assert mask.dtype == bool and np.array_equal(mask, want[cap][1])
        assert r.ExactKept()["cap"] == cap
    assert seen == list(caps) and r.ExactKept()["valid"] == 0
    # without the check the frames come with None, as render's do
    got = [(cap, mask) for cap, mask in exact.render_progressive(r, v, caps[:2], bailout=256, frac_bits=F)]
    assert got == [(200, None), (1000, None)]
    assert _frame(r, W, H, 1000).tobytes() == want[1000][0].tobytes()
