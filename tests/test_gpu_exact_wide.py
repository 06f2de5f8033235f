"""The wide exact renderer (fs_exact_sample_counts, fs_render_exact_wide, fs_exact_wide_state; one wave per sample, 2 .. 704 limbs)
on the GPU: its state after a few steps against the Python-integer recurrence on every limb, its counts against GMP integer
iteration (tests/_truth.py, run live) at every block size, against the narrow kernel where both exist, and against the exact-count
fixture."""
import random
import time

import numpy as np
import pytest

import _truth
from fractalshark_amd import GPURenderer, exact, inputs
from fractalshark_amd.renderer import FS_ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu

FS_ERR_6 = 10005
HIP_INVALID_VALUE = 1


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


def _render_wide(r, v, w, h, R, F, inclusive=False, iter_bytes=4, limbs=None):
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False, iter_bytes=iter_bytes) == 0
    assert r.ClearMemory() == 0
    L = exact.limbs_for(F) if limbs is None else limbs
    cx, cy = exact.axes(v, F, limbs=L)
    assert r.RenderExactWide(iter_bytes, F, L, cx, cy, R, inclusive, v.num_iterations) == 0
    return _frame(r, w, h, v.num_iterations)


def _render_narrow(r, v, w, h, R, F, inclusive=False):
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False) == 0
    assert r.ClearMemory() == 0
    cx, cy = exact.axes(v, F)
    assert r.RenderExact(4, F, exact.limbs_for(F), cx, cy, R, inclusive, v.num_iterations) == 0
    return _frame(r, w, h, v.num_iterations)


def _truth_frame(v, w, h, R, F, cap, inclusive=False):
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    E, _ = _truth.exact_counts(v.bbox(), w, h, gx.ravel(), gy.ravel(), cap + 1, R, F, shifts=[], inclusive=inclusive)
    return _truth.expect_minus_one(E, cap).reshape(h, w)


def _same(got, want, what):
    bad = int((np.asarray(got, np.int64) != want).sum())
    print("exact wide %-44s %d samples, %d differ" % (what, want.size, bad))
    assert bad == 0, (what, bad)


# ---- 1. the state, bit for bit
STATE_STEPS = (1, 2, 3, 40)
# limbs -> frac_bits: block sizes 1, 2, 3 and 11; full and ragged top lanes; r = 0 (2048, 4096) and r != 0; q on a lane boundary
# (2048 = 32 * 64 with one limb per lane... and two) and off it
STATE_F = {2: 54, 25: 790, 64: 2038, 65: 2048, 80: 2550, 128: 4086, 129: 4096, 683: 21829, 704: 22518}


def _state_samples(L, F):
    rng = random.Random(1000 + L)
    half = (1 << (16 * L)) - 1
    s = [(rng.randrange(-2 << F, 2 << F), rng.randrange(-2 << F, 2 << F)) for _ in range(16)]
    s += [(rng.randrange(-3 << (F - 1), 1 << (F - 1)), rng.randrange(-1 << F, 1 << F)) for _ in range(16)]  # |c| < 2, many stay
    s += [(-1, 0),                                   # -1 unit: every limb all ones
          (-2 << F, 0), ((-2 << F) + 1, 0), ((-2 << F) - 1, 0), (0, 1),
          (-(32 << F) + 1, 0), (-(32 << F), 0),      # the top of the range (kept: |c|^2 > 256)
          ((1 << (F - 2)) & ~half | half, 0),        # the low half all ones: a carry crosses every lane
          (-(1 << F) & ~half | half, (1 << (F - 3)) & ~half | half),
          (0, 0), (-(1 << F), 1), (-(3 << (F - 1)), -1)]
    return s


def _python_states(samples, F):
    """{steps: [(x, y)]}: the recurrence on Python integers, a z with |z|^2 > 256 kept as it is."""
    out = {k: [] for k in STATE_STEPS}
    bound = 256 << (2 * F)
    for cx, cy in samples:
        x, y = cx, cy
        for k in range(1, max(STATE_STEPS) + 1):
            xx, yy = x * x, y * y
            if xx + yy <= bound:
                x, y = ((xx - yy) >> F) + cx, ((2 * x * y) >> F) + cy
            if k in out:
                out[k].append((x, y))
    return out


def _planes(values, L):
    """Python integers -> uint32[L, n], two's complement, limb-major."""
    mask = (1 << (32 * L)) - 1
    rows = [np.frombuffer((v & mask).to_bytes(4 * L, "little"), np.uint32) for v in values]
    return np.ascontiguousarray(np.array(rows, np.uint32).T)


_state_cache = {}


def _state_case(L):
    if L not in _state_cache:
        F = STATE_F[L]
        s = _state_samples(L, F)
        _state_cache[L] = (F, s, _python_states(s, F))
    return _state_cache[L]


@pytest.mark.parametrize("L", sorted(STATE_F))
def test_state_equals_python_integers_on_every_limb(renderer, L):
    F, samples, want = _state_case(L)
    assert exact.limbs_for(F) == L or L == 2
    cx, cy = _planes([s[0] for s in samples], L), _planes([s[1] for s in samples], L)
    moved = 0
    for steps in STATE_STEPS:
        err, x, y = renderer.ExactWideState(F, L, cx, cy, steps)
        assert err == 0
        wx, wy = _planes([z[0] for z in want[steps]], L), _planes([z[1] for z in want[steps]], L)
        bad = np.flatnonzero(((x != wx) | (y != wy)).any(axis=0))
        print("exact wide state L %3d F %5d steps %2d: %d samples, %d differ%s" % (
            L, F, steps, len(samples), len(bad),
            "" if not len(bad) else " (first: sample %d, lowest limb %d)" % (bad[0], int(np.flatnonzero((x != wx)[:, bad[0]] | (y != wy)[:, bad[0]])[0]))))
        assert len(bad) == 0, (L, steps, bad.tolist())
        moved = sum(1 for z, c in zip(want[steps], samples) if z != c)
    assert moved >= len(samples) // 2  # most samples are still being stepped at the end


# ---- 2. counts at every width against live truth
def _shallow(w=16, h=9, cap=2000):
    b = _truth.Case("shallow_1e-6").raw["bbox"]
    return inputs.View(b[0], b[1], b[2], b[3], w, h, num_iterations=cap), w, h, cap


COUNT_CASES = [(256, F) for F in (759, 2038, 2048, 2550, 4086, 4087, 5100, 21829, 22518)] + [(4, 2550), (4, 21829)]
_truth_cache = {}


def _shallow_truth(R, F):
    if (R, F) not in _truth_cache:
        v, w, h, cap = _shallow()
        _truth_cache[(R, F)] = _truth_frame(v, w, h, R, F, cap)
    return _truth_cache[(R, F)]


@pytest.mark.parametrize("R,F", COUNT_CASES)
def test_counts_equal_live_truth_at_every_width(renderer, R, F):
    v, w, h, cap = _shallow()
    want = _shallow_truth(R, F)
    assert int((want < cap).sum()) > want.size // 2
    t0 = time.time()
    got = _render_wide(renderer, v, w, h, R, F)
    print("exact wide F %5d (%3d limbs) R%d: %.2f s, %s" % (F, exact.limbs_for(F), R, time.time() - t0, renderer.exact_stats()))
    _same(got, want, "shallow_1e-6 16x9 at F %d, R%d" % (F, R))


# ---- 3. wide equals narrow where both exist
@pytest.mark.parametrize("R", [4, 256])
@pytest.mark.parametrize("name", ["shallow_1e-12", "shallow_1e-28", "x2_c0_1e-40"])
def test_wide_frame_is_the_narrow_frame(renderer, name, R):
    c = _truth.Case(name)
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    assert exact.limbs_for(F) <= exact.MAX_LIMBS
    narrow = _render_narrow(renderer, v, c.w, c.h, R, F).copy()
    wide = _render_wide(renderer, v, c.w, c.h, R, F).copy()
    assert wide.tobytes() == narrow.tobytes(), (name, R, int((wide != narrow).sum()))


# ---- 4. strict and inclusive bailout on samples that land on R exactly
@pytest.mark.parametrize("F", [759, 2048])
@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("bbox,R", [(_truth.BOUNDARY_BBOX, 4), (_truth.BOUNDARY_BBOX_256, 256)])
def test_boundary_views(renderer, bbox, R, inclusive, F):
    v = _truth.boundary_view(inputs, bbox)
    n, cap = _truth.BOUNDARY_SIZE, _truth.BOUNDARY_CAP
    got = _render_wide(renderer, v, n, n, R, F, inclusive=inclusive)
    _same(got, _truth_frame(v, n, n, R, F, cap, inclusive=inclusive), "boundary R%d inclusive=%s F %d" % (R, inclusive, F))
    if R == 4:
        (x0, y0), (x1, y1) = _truth.BOUNDARY_SAMPLES
        assert (int(got[y0, x0]), int(got[y1, x1])) == ((0, 0) if inclusive else (1, cap))
    else:
        x, y = _truth.BOUNDARY_CENTRE
        assert int(got[y, x]) == (0 if inclusive else 1)


# ---- 5. slices
def test_slicing_and_buffer_width_change_nothing(renderer):
    r = renderer
    v, w, h, cap = _shallow()
    F = 2550
    base = _render_wide(r, v, w, h, 256, F).copy()
    one = r.exact_stats()
    longest = int(base.max()) + 1
    assert longest == cap + 1  # (two samples of the frame never escape)
    assert one["lane_steps"] == int(base.astype(np.int64).sum()) + base.size and one["lane_slots"] == 64 * one["lane_steps"]
    try:
        assert r.SetExactSlice(16) == 0
        sliced = _render_wide(r, v, w, h, 256, F).copy()
        many = r.exact_stats()
        assert many["launches"] == -(-longest // 16) and many["lane_steps"] == one["lane_steps"]
        wide = _render_wide(r, v, w, h, 256, F, iter_bytes=8).copy()
    finally:
        r.SetExactSlice(0)
    assert sliced.tobytes() == base.tobytes()
    assert wide.dtype == np.uint64 and np.array_equal(wide, base)
    _same(base, _shallow_truth(256, F), "shallow_1e-6 16x9 at F 2550 (default slice)")


# ---- 6. sample_counts with a stability ladder against the fixture
@pytest.mark.parametrize("R", [4, 256])
def test_sample_counts_and_stability_bits_equal_the_fixture(renderer, R):
    c = _truth.Case("shallow_1e-20")
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    assert len(c.ladder) == 8
    t0 = time.time()
    values, stable = exact.sample_counts(renderer, v, c.xs, c.ys, bailout=R, frac_bits=F, levels=c.ladder)
    print("exact wide sample_counts shallow_1e-20 R%d: %d samples, 8 levels, %.2f s" % (R, len(c.xs), time.time() - t0))
    assert values.dtype == np.int64 and stable.shape == (len(c.xs), 8) and stable.dtype == bool
    _same(values, _truth.expect_minus_one(c.counts(R), c.cap), "shallow_1e-20 R%d fixture samples" % R)
    for j, level in enumerate(c.ladder):
        bad = int((stable[:, j] != c.stable(R, level)).sum())
        assert bad == 0, (R, level, bad)


# ---- 7. View 11: 2 550 fractional bits, 80 limbs
def test_view11_fixture_samples(renderer):
    """The fixture's 200 samples at a cap above the largest count; the two that never escape return the cap.  This is the suite's
    longest test by far, 714 399 steps of a lone wave: the time it took is in DESIGN.md 6.3 "Wide"."""
    c = _truth.Case("view11_64x36")
    v, F = c.view(inputs), c.raw["frac_bits"]
    E = c.counts(256)
    cap = 720000
    assert F == 2550 and len(c.xs) == 200 and int(E.max()) == 714399 and int((E == 0).sum()) == 2 and cap > int(E.max())
    v.num_iterations = cap
    t0 = time.time()
    values, _ = exact.sample_counts(renderer, v, c.xs, c.ys, bailout=256, frac_bits=F)
    print("exact wide view11_64x36: 200 samples at cap %d in %.2f s (%s); the GMP counter took %.0f s" % (
        cap, time.time() - t0, renderer.exact_stats(), c.raw["generator_seconds"]))
    assert (values[E == 0] == cap).all()
    _same(values, _truth.expect_minus_one(E, cap), "view11_64x36 R256 fixture samples")


# ---- 8. what is refused, and what is left alone
def test_error_returns(renderer):
    r = renderer
    z = lambda L, n: np.zeros((L, n), np.uint32)
    fresh = GPURenderer(0)
    try:
        err, out = fresh.ExactSampleCounts(2550, 80, z(80, 3), z(80, 3), 4, False, 50)  # no InitializeMemory needed
        assert err == 0 and out.tolist() == [50, 50, 50]
        assert fresh._lib.fs_render_exact_wide(fresh._h, 4, 2550, 80, z(80, 64).ctypes.data, z(80, 36).ctypes.data, 4, 0, 100) == FS_ERR_6
        assert fresh._lib.fs_render_exact_wide(fresh._h, 4, 2550, 79, z(79, 64).ctypes.data, z(79, 36).ctypes.data, 4, 0, 100) == FS_ERR_6  # no frame, bad limbs
    finally:
        fresh.close()

    def counts(F=2550, L=80, R=4, n=100, x=None, y=None):
        x = z(L, 4) if x is None else x
        y = z(L, 4) if y is None else y
        return r._lib.fs_exact_sample_counts(r._h, F, L, x.ctypes.data, y.ctypes.data, x.shape[1], R, 0, n, np.zeros(x.shape[1], np.uint64).ctypes.data)

    assert counts() == 0
    assert counts(L=705, F=22518) == FS_ERR_UNSUPPORTED
    assert counts(L=704, F=22519) == FS_ERR_UNSUPPORTED and counts(L=704, F=22518) == 0
    assert counts(L=79) == FS_ERR_UNSUPPORTED          # 32 * 79 < 2550 + 10
    assert counts(L=1, F=10) == FS_ERR_UNSUPPORTED
    assert counts(R=0) == FS_ERR_UNSUPPORTED and counts(R=257) == FS_ERR_UNSUPPORTED and counts(R=256) == 0 and counts(R=1) == 0
    far = z(80, 4)
    limbs_of = lambda v: [(v >> (32 * l)) & 0xFFFFFFFF for l in range(80)]
    far[:, 3] = limbs_of(32 << 2550)                  # c = 32
    assert counts(x=far) == FS_ERR_UNSUPPORTED and counts(y=far) == FS_ERR_UNSUPPORTED
    far[:, 3] = limbs_of(-32 << 2550)                 # c = -32 is inside
    assert counts(x=far) == 0
    far[:, 3] = limbs_of((-32 << 2550) - 1)
    assert counts(x=far) == FS_ERR_UNSUPPORTED
    assert r.ExactWideState(2550, 79, z(79, 4), z(79, 4), 1)[0] == FS_ERR_UNSUPPORTED
    # two faults at once: the first refusal in the header's order decides
    raw = lambda L=80, n_samples=4, cap=100, x=None, y=None, out=None: r._lib.fs_exact_sample_counts(r._h, 2550, L, x, y, n_samples, 4, 0, cap, out)
    zero4, out4 = z(80, 4), np.zeros(4, np.uint64)
    far[:, 3] = limbs_of(32 << 2550)
    assert counts(L=79, n=(1 << 64) - 1) == FS_ERR_UNSUPPORTED                       # the format before the cap
    assert raw(n_samples=0, cap=(1 << 64) - 1, x=zero4.ctypes.data, y=zero4.ctypes.data, out=out4.ctypes.data) == HIP_INVALID_VALUE  # the cap before "no samples"
    assert raw(n_samples=0) == 0                                                     # "no samples" before the NULL arrays
    assert raw(x=far.ctypes.data, y=zero4.ctypes.data, out=None) == HIP_INVALID_VALUE  # a NULL array before the axis range

    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False) == 0
    cx, cy = z(80, 64), z(80, 36)
    frame = lambda ib=4, F=2550, L=80, R=4, n=100, x=cx, y=cy: r._lib.fs_render_exact_wide(r._h, ib, F, L, x.ctypes.data, y.ctypes.data, R, 0, n)
    assert frame() == 0
    assert frame(L=705, F=22518, x=z(705, 64), y=z(705, 36)) == FS_ERR_UNSUPPORTED
    assert frame(L=79) == FS_ERR_UNSUPPORTED and frame(L=1, F=10) == FS_ERR_UNSUPPORTED
    assert frame(R=0) == FS_ERR_UNSUPPORTED and frame(R=257) == FS_ERR_UNSUPPORTED
    assert frame(ib=2) == FS_ERR_UNSUPPORTED
    assert frame(ib=8) == HIP_INVALID_VALUE            # the frame holds 4-byte counts
    assert frame(n=1 << 32) == HIP_INVALID_VALUE       # a cap that a 4-byte frame cannot hold
    farx = cx.copy()
    farx[:, 3] = limbs_of(32 << 2550)
    assert frame(x=farx) == FS_ERR_UNSUPPORTED
    # two faults at once
    assert frame(ib=2, n=1 << 32) == FS_ERR_UNSUPPORTED  # iter_bytes before the cap (fs_render_exact: after it)
    assert frame(L=79, n=1 << 32) == FS_ERR_UNSUPPORTED  # the format before the cap
    assert frame(ib=8, x=farx) == HIP_INVALID_VALUE      # the frame's iter_bytes before the axis range
    farx[:, 3] = limbs_of(-32 << 2550)
    assert frame(x=farx) == 0
    # the narrow entry points still end at 24 limbs
    assert r._lib.fs_render_exact(r._h, 4, 790, 25, z(25, 64).ctypes.data, z(25, 36).ctypes.data, 4, 0, 100) == FS_ERR_UNSUPPORTED
    assert r.SetRowBands(0, 8, 16) == 0
    try:
        assert frame() == FS_ERR_UNSUPPORTED
    finally:
        assert r.SetRowBands(0, 0, 0) == 0


def test_frame_state_is_left_as_it_was(renderer):
    """An orbit and an LA table resident before a wide call render the same LAv2 frame after it; fs_exact_sample_counts does not
    touch the frame at all."""
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
    v0.num_iterations = 300
    values, _ = exact.sample_counts(r, v0, [0, 20, 63], [0, 18, 35], frac_bits=790)
    assert values.shape == (3,)
    assert _frame(r, 64, 36, v.num_iterations).tobytes() == before.tobytes()
    exact.render(r, v0, frac_bits=790)  # 25 limbs: the wide frame call
    after = _frame(r, 64, 36, v0.num_iterations)
    assert not np.array_equal(after, before)
    assert [int(after[y, x]) for x, y in ((0, 0), (20, 18), (63, 35))] == values.tolist()
    assert lav2() == 0
    assert _frame(r, 64, 36, v.num_iterations).tobytes() == before.tobytes()


def test_zoom_loop_goes_on_past_the_narrow_limit(renderer):
    """autozoom.zoom with exact.render from a view that already needs 25 limbs: the step that used to end in FS_ERR_UNSUPPORTED
    renders, and equals live truth."""
    from fractalshark_amd import autozoom
    r = renderer
    w, h = 16, 9
    b = _truth.Case("shallow_1e-6").raw["bbox"]
    from fractions import Fraction
    minx, miny, maxx, maxy = (Fraction(t) for t in b)
    cxm, cym = minx + (maxx - minx) * 3 / 16, maxy - (maxy - miny) * 2 / 9  # a sample of the 16 x 9 frame that escapes
    half = Fraction(1, 1 << 700)
    dec = lambda q: "%se-400" % ((q * 10 ** 400).numerator // (q * 10 ** 400).denominator)
    view = inputs.View(dec(cxm - half), dec(cym - half * 9 / 16), dec(cxm + half), dec(cym + half * 9 / 16), w, h, num_iterations=500)
    assert exact.uses_wide(exact.limbs_for(view.precision_bits + exact.GUARD_BITS))
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False) == 0
    steps = 0
    for v, picked, nv in autozoom.zoom(r, view, autozoom.MAX, exact.render, 2):
        F = v.precision_bits + exact.GUARD_BITS
        assert exact.limbs_for(F) > exact.MAX_LIMBS
        want = _truth_frame(v, w, h, 4, F, v.num_iterations)
        assert 0 < int(want.max()) < v.num_iterations
        _same(_frame(r, w, h, v.num_iterations), want, "zoom step %d (F %d)" % (steps, F))
        steps += 1
    assert steps >= 1
