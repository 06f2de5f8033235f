"""The exact renderer (fs_render_exact, fs_exact_stable_mask; fractalshark_amd.exact) on the GPU against GMP integer iteration of
the same recurrence (tests/_truth.py, run live) and the exact-count fixture: equality on EVERY compared sample, stable or not --
nothing in this path is rounded, so there is no stability level to choose and no sample to leave out."""
import ctypes as C

import numpy as np
import pytest

import _truth
from fractalshark_amd import GPURenderer, _capi, autozoom, exact, inputs
from fractalshark_amd.renderer import FS_ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu

FS_ERR_6 = 10005
HIP_INVALID_VALUE = 1
FX = _truth.fixture()["cases"]
GENERATED = sorted(k for k in FX if k.startswith("shallow_") or k.startswith("x2_"))


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.SetExactSlice(0)
    r.close()


def _frame(r, w, h, n):
    out = r.new_iter_buffer()
    assert r.RenderCurrent(n, out) == 0
    assert r.SyncComputeStream() == 0
    return out[:h, :w]


def _render(r, v, w, h, R, F, inclusive=False, iter_bytes=4):
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False, iter_bytes=iter_bytes) == 0
    assert r.ClearMemory() == 0
    exact.render(r, v, bailout=R, frac_bits=F, iter_bytes=iter_bytes, inclusive=inclusive)
    return _frame(r, w, h, v.num_iterations)


def _truth_frame(v, w, h, R, F, cap, inclusive=False):
    """min(E - 1, N) of every pixel from GMP integer iteration, limit = cap + 1."""
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    E, _ = _truth.exact_counts(v.bbox(), w, h, gx.ravel(), gy.ravel(), cap + 1, R, F, shifts=[], inclusive=inclusive)
    return _truth.expect_minus_one(E, cap).reshape(h, w)


def _same(got, want, what):
    bad = int((np.asarray(got, np.int64) != want).sum())
    print("exact %-40s %d pixels, %d differ" % (what, want.size, bad))
    assert bad == 0, (what, bad)


@pytest.mark.parametrize("R", [4, 256])
@pytest.mark.parametrize("name", GENERATED)
def test_whole_frame_equals_live_truth(renderer, name, R):
    c = _truth.Case(name)
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    _same(_render(renderer, v, c.w, c.h, R, F), _truth_frame(v, c.w, c.h, R, F, c.cap), "%s R%d" % (name, R))


def test_view0_full_size_frame_and_reductions(renderer):
    c = _truth.Case("view0_1024x768")
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    got = _render(renderer, v, c.w, c.h, 4, F)
    assert len(c.xs) == 825
    _same(c.sample(got), _truth.expect_minus_one(c.counts(4), c.cap), "view0_1024x768 R4 fixture samples")
    red = _capi.Reduction()
    assert renderer.RenderCurrent(c.cap, None, None, red) == 0 and renderer.SyncComputeStream() == 0
    g = got.astype(np.uint64)
    assert (red.Min, red.Max, red.Sum) == (int(g.min()), int(g.max()), int(g.sum()))


@pytest.mark.parametrize("name,R", [("view3_64x36", 256), ("view5_64x36", 256), ("view5_64x36", 4)])
def test_deep_views_at_the_fixture_cap(renderer, name, R):
    """View 5's cap is 4.7 million: a never-escaping sample runs through more than a thousand slices."""
    c = _truth.Case(name)
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    got = _render(renderer, v, c.w, c.h, R, F)
    _same(c.sample(got), _truth.expect_minus_one(c.counts(R), c.cap), "%s R%d fixture samples" % (name, R))
    longest = int(np.where(c.counts(R) == 0, c.cap + 1, c.counts(R)).max())  # (two of View 5's samples never escape)
    assert renderer.exact_stats()["launches"] >= -(-longest // 4096)


def test_view19_largest_instantiation(renderer):
    """F = 707: 23 limbs."""
    w, h, cap = 64, 36, 20000
    v = inputs.View.builtin(19, w, h, antialiasing=1)
    v.num_iterations = cap
    F = v.precision_bits + _truth.GUARD_BITS
    assert F == 707 and exact.limbs_for(F) == 23
    _same(_render(renderer, v, w, h, 256, F), _truth_frame(v, w, h, 256, F, cap), "view19_64x36 R256")


def test_largest_instantiation_on_samples_that_escape(renderer):
    """Every sample of View 19 at 64 x 36 sits at a cap of 20 000, so the frame above says little about 23-limb arithmetic beyond
    "nothing escaped".  shallow_1e-6 rendered with the same 707 fractional bits escapes almost everywhere."""
    c = _truth.Case("shallow_1e-6")
    v, F = c.view(inputs), 707
    v.num_iterations = c.cap
    want = _truth_frame(v, c.w, c.h, 256, F, c.cap)
    assert int((want < c.cap).sum()) > want.size // 2
    _same(_render(renderer, v, c.w, c.h, 256, F), want, "shallow_1e-6 at F 707, R256")


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("bbox,R", [(_truth.BOUNDARY_BBOX, 4), (_truth.BOUNDARY_BBOX_256, 256)])
def test_boundary_views(renderer, bbox, R, inclusive):
    """|z|^2 lands on R exactly: c = 2i and c = -2 at R = 4, c = -16 at R = 256."""
    v = _truth.boundary_view(inputs, bbox)
    n, cap = _truth.BOUNDARY_SIZE, _truth.BOUNDARY_CAP
    F = v.precision_bits + _truth.GUARD_BITS
    got = _render(renderer, v, n, n, R, F, inclusive=inclusive)
    _same(got, _truth_frame(v, n, n, R, F, cap, inclusive=inclusive), "boundary R%d inclusive=%s" % (R, inclusive))
    if R == 4:
        (x0, y0), (x1, y1) = _truth.BOUNDARY_SAMPLES
        assert (int(got[y0, x0]), int(got[y1, x1])) == ((0, 0) if inclusive else (1, cap))
    else:
        x, y = _truth.BOUNDARY_CENTRE
        assert int(got[y, x]) == (0 if inclusive else 1)


def test_slicing_and_buffer_width_change_nothing(renderer):
    r = renderer
    c = _truth.Case("shallow_1e-12")
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    base = _render(r, v, c.w, c.h, 256, F).copy()
    one = r.exact_stats()
    longest = int(base.max()) + 1  # steps of the longest sample (the fixture's longest escapes at 5330)
    assert longest >= 5330 and one["launches"] == -(-longest // 4096) and one["lane_steps"] <= one["lane_slots"]
    try:
        assert r.SetExactSlice(16) == 0
        sliced = _render(r, v, c.w, c.h, 256, F).copy()
        many = r.exact_stats()
        assert many["launches"] == -(-longest // 16) >= 200 and many["lane_steps"] == one["lane_steps"]
        assert r.SetExactSlice(16, no_compaction=True) == 0
        loose = _render(r, v, c.w, c.h, 256, F).copy()
        assert r.exact_stats()["lane_steps"] == one["lane_steps"]
        assert r.SetExactSlice(16) == 0
        wide = _render(r, v, c.w, c.h, 256, F, iter_bytes=8).copy()
    finally:
        r.SetExactSlice(0)
    assert sliced.tobytes() == base.tobytes() == loose.tobytes()
    assert wide.dtype == np.uint64 and np.array_equal(wide, base)


@pytest.mark.parametrize("R", [4, 256])
def test_stable_mask_equals_the_fixture(renderer, R):
    c = _truth.Case("shallow_1e-20")
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    assert len(c.ladder) == 8
    centre = _render(renderer, v, c.w, c.h, R, F).copy()
    for level in c.ladder:
        mask = exact.stable_mask(renderer, v, level, bailout=R, frac_bits=F)
        want = c.stable(R, level)
        bad = int((mask[c.ys, c.xs] != want).sum())
        print("exact stable mask R%d level 2^-%d: %d of %d samples stable, %d differ" % (R, level, int(want.sum()), len(want), bad))
        assert bad == 0, (R, level, bad)
    assert _frame(renderer, c.w, c.h, c.cap).tobytes() == centre.tobytes()  # the centre frame is left alone


def test_zoom_loop_needs_no_orbit(renderer):
    """autozoom.zoom with exact.render and Max for 12 steps from View 0 at 64 x 36 -- past binary64, no orbit, no LA table -- and
    every frame it yields equals live truth on every pixel.

    One call of autozoom.zoom does not run 12 steps from this view, whatever the renderer or the cap: Max heads for the topmost
    sample inside the set, and the third frame already holds 543 samples at the cap (caps 256 .. 131072 all give 133, 9 or 10, then
    543 .. 563), above the reference's num_at_max > 500 at which the AutoZoomer moves once more and stops (AutoZoomer.cpp, kept by
    autozoom.zoom).  So the loop is started again from the view it stopped at, as a user would: twelve frames all the same, each one
    rendered and picked inside autozoom.zoom."""
    r = renderer
    w, h, want_steps = 64, 36, 12
    view = inputs.View.builtin(0, w, h, antialiasing=1)
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False) == 0
    steps, runs = 0, 0
    while steps < want_steps and view is not None:
        runs += 1
        start, nxt = steps, None
        for v, picked, nv in autozoom.zoom(r, view, autozoom.MAX, exact.render, want_steps - steps):
            F = v.precision_bits + exact.GUARD_BITS
            _same(_frame(r, w, h, v.num_iterations), _truth_frame(v, w, h, 4, F, v.num_iterations),
                  "zoom step %d (F %d, status %d, %d at the cap)" % (steps, F, picked.status, picked.num_at_max))
            steps, nxt = steps + 1, nv
        assert steps > start
        view = nxt
    print("exact zoom: %d steps in %d runs of autozoom.zoom" % (steps, runs))
    assert steps == want_steps
    assert view.precision_bits >= 120 + 3 + 40  # 12 steps of x16 from a view four units wide


def test_error_returns(renderer):
    fresh = GPURenderer(0)
    cx, cy = np.zeros((7, 64), np.uint32), np.zeros((7, 36), np.uint32)
    try:
        assert fresh._lib.fs_render_exact(fresh._h, 4, 187, 7, cx.ctypes.data, cy.ctypes.data, 4, 0, 100) == FS_ERR_6
        assert fresh._lib.fs_render_exact(fresh._h, 4, 187, 6, cx.ctypes.data, cy.ctypes.data, 4, 0, 100) == FS_ERR_6  # no frame, bad limbs
    finally:
        fresh.close()
    r = renderer
    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False) == 0
    call = lambda ib=4, F=187, L=7, R=4, n=100, x=cx, y=cy: r._lib.fs_render_exact(r._h, ib, F, L, x.ctypes.data, y.ctypes.data, R, 0, n)
    assert call() == 0
    assert call(L=6) == FS_ERR_UNSUPPORTED            # 32 * 6 < 187 + 10
    assert call(F=759, L=24) == FS_ERR_UNSUPPORTED    # beyond the largest instantiation
    assert call(F=790, L=25, x=np.zeros((25, 64), np.uint32), y=np.zeros((25, 36), np.uint32)) == FS_ERR_UNSUPPORTED
    assert call(L=1, F=10) == FS_ERR_UNSUPPORTED
    assert call(R=0) == FS_ERR_UNSUPPORTED and call(R=257) == FS_ERR_UNSUPPORTED and call(R=256) == 0 and call(R=1) == 0
    assert call(ib=2) == FS_ERR_UNSUPPORTED
    assert call(ib=8) == HIP_INVALID_VALUE            # the frame holds 4-byte counts
    assert call(n=1 << 32) == HIP_INVALID_VALUE
    far = cx.copy()
    far[:, 3] = [(32 << 187 >> (32 * l)) & 0xFFFFFFFF for l in range(7)]  # c = 32
    assert call(x=far) == FS_ERR_UNSUPPORTED
    # two faults at once: the first refusal in the header's order decides
    assert call(ib=2, n=1 << 32) == HIP_INVALID_VALUE   # the cap comes before iter_bytes (fs_render_exact_wide: after it)
    assert r._lib.fs_render_exact(r._h, 2, 187, 7, None, cy.ctypes.data, 4, 0, 100) == FS_ERR_UNSUPPORTED  # iter_bytes before a NULL axis
    assert call(L=6, n=1 << 32) == FS_ERR_UNSUPPORTED   # the format before the cap
    assert call(ib=8, x=far) == HIP_INVALID_VALUE       # the frame's iter_bytes before the axis range
    ptrs = lambda a3: (C.c_void_p * 3)(*[a.ctypes.data if a is not None else None for a in a3])
    mask = np.zeros((36, 64), np.uint8)
    stable = lambda x3, y3, R=4, n=100: r._lib.fs_exact_stable_mask(r._h, 187, 7, ptrs(x3), ptrs(y3), R, n, mask.ctypes.data)
    zx, zy = np.zeros((7, 64), np.uint32), np.zeros((7, 36), np.uint32)
    assert stable([zx, zx, zx], [zy, zy, zy]) == 0
    assert stable([zx, None, zx], [zy, zy, zy], R=300) == FS_ERR_UNSUPPORTED  # the format before a NULL axis
    assert stable([far, zx, zx], [zy, zy, zy], n=1 << 32) == HIP_INVALID_VALUE  # the cap before the axis range
    far[:, 3] = [((-32 << 187) >> (32 * l)) & 0xFFFFFFFF for l in range(7)]  # c = -32 is inside
    assert call(x=far) == 0
    far[:, 3] = [(((-32 << 187) - 1) >> (32 * l)) & 0xFFFFFFFF for l in range(7)]
    assert call(x=far) == FS_ERR_UNSUPPORTED
    cx3, cy3 = np.zeros((3, 7, 64), np.uint32), np.zeros((3, 7, 36), np.uint32)
    assert r.ExactStableMask(187, 7, cx3, cy3, 4, 100)[0] == 0
    assert r.ExactStableMask(187, 7, cx3, cy3, 300, 100)[0] == FS_ERR_UNSUPPORTED
    assert r.SetRowBands(0, 8, 16) == 0
    try:
        assert call() == FS_ERR_UNSUPPORTED
        assert call(n=1 << 32) == FS_ERR_UNSUPPORTED    # row bands before the cap
        assert r.ExactStableMask(187, 7, cx3, cy3, 4, 100)[0] == FS_ERR_UNSUPPORTED
    finally:
        assert r.SetRowBands(0, 0, 0) == 0


def test_frame_state_is_left_as_it_was(renderer):
    """An orbit and an LA table resident before an exact frame render the same LAv2 frame after it."""
    from fractalshark_amd import LAV2_FULL, PARITY_CPU, T_HDR32
    r = renderer
    v = inputs.View.builtin(5, 64, 36)
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False) == 0
    assert r.InitializePerturb(7, ob, 0, None, la) == 0
    co = [(float(c["m"]), int(c["e"])) for c in v.coords_perturb_hdr32(ob)]
    lav2 = lambda: r.RenderPerturbLAv2(None, None, None, *co, v.num_iterations, T=T_HDR32, Mode=LAV2_FULL, parity=PARITY_CPU)
    assert lav2() == 0
    before = _frame(r, 64, 36, v.num_iterations).copy()
    v0 = inputs.View.builtin(0, 64, 36, antialiasing=1)
    exact.render(r, v0)
    assert not np.array_equal(_frame(r, 64, 36, v0.num_iterations), before)
    assert lav2() == 0
    assert _frame(r, 64, 36, v.num_iterations).tobytes() == before.tobytes()
