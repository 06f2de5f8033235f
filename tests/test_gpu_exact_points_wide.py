"""Point runs on the wide path (fs_exact_eval_points_wide; exact.eval_points(wide=True)): values, atom periods and every limb of
every endpoint against the definitions on Python integers (tests/_point_model.py) beyond the lane path's 24 limbs, and against the
lane path byte for byte where both run.  No tolerance anywhere: the device evaluates the exact recurrence."""
from fractions import Fraction

import numpy as np
import pytest

import _point_model as model
from fractalshark_amd import GPURenderer, exact, inputs

pytestmark = pytest.mark.gpu

FS_ERR_UNSUPPORTED, INVALID = 10100, 1  # (hipErrorInvalidValue)
# (the points of tests/test_gpu_exact_points.py: c = 0, -1, 1/4, next to the period-3 nucleus, (35/2, 1/3) which escapes at once)
POINTS = [(0, 0), (-1, 0), (Fraction(1, 4), 0), (Fraction(5, 2), Fraction(1, 3)), (-2, 0), (Fraction(-3, 4), Fraction(1, 20)),
          (Fraction(-12253, 100000), Fraction(74484, 100000)), (Fraction(35, 2), Fraction(1, 3)), (Fraction(-1, 2), Fraction(1, 2)),
          (Fraction(3, 10), Fraction(1, 2)), (Fraction(-7, 4), Fraction(1, 1000)), (Fraction(-3, 4), Fraction(1, 100)),
          (Fraction(28, 100), Fraction(1, 100))]
EDGE = POINTS[12]  # escapes after a few dozen steps at every bailout: the runs around its escape index are made of it
LENGTHS = (1, 2, 3, 64, 65, 1000)  # (13 points, 6 lengths: every pair comes up over 78 runs)
LENGTHS_DEEP = (1, 2, 3, 40)       # 683 and 704 limbs, where a step takes 165 us: every pair over 52 runs
LANE_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 100, 333, 1000)


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _switches_off(renderer):
    yield
    assert renderer.SetExactPeriods(False) == 0 and renderer.SetExactCycleCheck(False) == 0 and renderer.SetExactKeep(False) == 0
    assert renderer.SetExactSlice(0) == 0


_cache = {}


def _runs(F, R, inclusive, lengths, n):
    """(cxs, cys, lengths, model results), once per configuration and never changed: n runs, the points in turn and the lengths in
    turn, then three runs of EDGE whose lengths are E - 1, E and E + 1, E the index at which it escapes: the escape comes one step
    after the length (z_{p+1} is tested, the run keeps its endpoint), at the length and before it."""
    key = (F, R, inclusive, lengths, n)
    if key not in _cache:
        cxs = [model.fix(POINTS[k % len(POINTS)][0], F) for k in range(n)]
        cys = [model.fix(POINTS[k % len(POINTS)][1], F) for k in range(n)]
        ps = [lengths[k % len(lengths)] for k in range(n)]
        ex, ey = model.fix(EDGE[0], F), model.fix(EDGE[1], F)
        E = model.run(ex, ey, F, R, inclusive, 1000)[0] + 1
        assert 3 < E < 60
        cxs, cys, ps = cxs + [ex] * 3, cys + [ey] * 3, ps + [E - 1, E, E + 1]
        want = [model.run(a, b, F, R, inclusive, p) for a, b, p in zip(cxs, cys, ps)]
        assert want[-3][0] == E - 1 and want[-3][2] is not None and want[-2][::2] == (E - 1, None) and want[-1][::2] == (E - 1, None)
        _cache[key] = (cxs, cys, ps, want)
    return _cache[key]


def _check(r, L, R, inclusive, what, lengths=LENGTHS, n=78):
    """One raw call at L limbs and F = 32 L - 10 against the model: values, atoms, every limb of every endpoint (all zero for a run
    short of its length), and the statistics.  Returns (outputs as bytes, statistics)."""
    F = 32 * L - 10
    assert exact.limbs_for(F) == L
    cxs, cys, ps, want = _runs(F, R, inclusive, lengths, n)
    err, values, atoms, end_x, end_y = r.ExactEvalPointsWide(F, L, exact._to_limbs(cxs, L), exact._to_limbs(cys, L),
                                                             np.array(ps, np.uint64), R, inclusive)
    assert err == 0 and end_x.shape == end_y.shape == (L, len(ps))
    xs, ys = exact._from_limbs(end_x), exact._from_limbs(end_y)
    got = [(int(v), int(a), (x, y) if w[2] is not None else None) for v, a, x, y, w in zip(values, atoms, xs, ys, want)]
    bad = [k for k in range(len(ps)) if got[k] != want[k]]
    short = [k for k, w in enumerate(want) if w[2] is None]
    print("wide points %-40s %d runs, %d short of their length, %d differ from the model" % (what, len(ps), len(short), len(bad)))
    assert not bad, (what, bad[:4], [(got[k][:2], want[k][:2], ps[k]) for k in bad[:3]])
    for k in short:
        assert not end_x[:, k].any() and not end_y[:, k].any(), (what, k)
    assert 5 < len(short) < len(ps) - 20 and any(w[0] == 0 for w in want) and len({w[1] for w in want}) > 5
    st = r.exact_stats()
    steps = sum(w[0] + 1 for w in want)  # a run makes v + 1 escape tests, a wave step each
    assert (st["lane_steps"], st["lane_slots"]) == (steps, 64 * steps) and st["launches"] >= 1, (what, st, steps)
    return (values.tobytes(), atoms.tobytes(), end_x.tobytes(), end_y.tobytes()), st


@pytest.mark.parametrize("L", [25, 64, 65, 80, 128, 129])
def test_runs_equal_the_model(renderer, L):
    """81 runs in one call, lengths 1 .. 1000 mixed, runs that escape before, at and one step after their length among runs that do
    not: the first limb count past the lane path, both sides of 64 and of 128 limbs (1, 2 and 3 limbs per lane), View 11's 80."""
    assert exact.uses_wide(L)
    _check(renderer, L, 256, False, "L %d" % L)


@pytest.mark.parametrize("L", [683, 704])
def test_deep_runs_equal_the_model(renderer, L):
    """View 14's 683 limbs and the most there is, 11 limbs per lane: lengths 1, 2, 3 and 40 and the three runs around the escape."""
    _check(renderer, L, 256, False, "L %d" % L, LENGTHS_DEEP, 52)


@pytest.mark.parametrize("L", [25, 80])
@pytest.mark.parametrize("R,inclusive", [(4, False), (256, True), (4, True)])
def test_bailouts_and_the_inclusive_test(renderer, L, R, inclusive):
    _check(renderer, L, R, inclusive, "L %d R %d incl %d" % (L, R, inclusive))


@pytest.mark.parametrize("F", [54, 246, 758])
def test_the_two_paths_agree_byte_for_byte(renderer, F):
    """exact.eval_points with wide=True and without, 130 runs with lengths 1 .. 1000 mixed at 2, 8 and 24 limbs: values, atoms and
    all endpoint limbs -- the raw planes of both entry points too."""
    r, n = renderer, 130
    L = exact.limbs_for(F)
    assert L == {54: 2, 246: 8, 758: 24}[F]
    cxs = [model.fix(POINTS[k % len(POINTS)][0], F) for k in range(n)]
    cys = [model.fix(POINTS[k % len(POINTS)][1], F) for k in range(n)]
    ps = [LANE_LENGTHS[k % len(LANE_LENGTHS)] for k in range(n)]
    lane = exact.eval_points(r, cxs, cys, ps, F, wide=False)
    wide = exact.eval_points(r, cxs, cys, ps, F, wide=True)
    assert wide == lane
    assert 10 < sum(1 for e in lane[2] if e is None) < n - 40 and len(set(lane[1])) > 8
    args = (F, L, exact._to_limbs(cxs, L), exact._to_limbs(cys, L), np.array(ps, np.uint64), 256, False)
    a, b = r.ExactEvalPoints(*args), r.ExactEvalPointsWide(*args)
    assert a[0] == b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("L", [25, 129])
def test_slices(renderer, L):
    """Slices of 1, of 16 and the default: the same bytes.  Runs of different lengths leave the list at different slices, the
    compaction moves the others to new slots, and every slice reads the run's minimum back from the planes by the run's index."""
    r = renderer
    base, st0 = _check(r, L, 256, False, "L %d default slice" % L)
    assert st0["launches"] == 1
    for steps in (16, 1):
        assert r.SetExactSlice(steps, False) == 0
        out, st = _check(r, L, 256, False, "L %d slice %d" % (L, steps))
        assert out == base
        assert st["launches"] == (1000 + 1 + steps - 1) // steps and st["lane_steps"] == st0["lane_steps"]
        assert 0 < st["running_after_first_slice"] < 81


def test_ties_go_to_the_earliest(renderer):
    """c = 0: every N_n is 0, so A = 1 at any length.  c = -1: N is 0 at n = 2, 4 and 6, so a run of 6 has A = 2."""
    r = renderer
    for L in (25, 80):
        F = 32 * L - 10
        for steps in (0, 1):
            assert r.SetExactSlice(steps, False) == 0
            values, atoms, ends = exact.eval_points(r, [0, 0, 0, -1 << F, -1 << F], [0] * 5, [1, 7, 100, 6, 5], F, wide=True)
            assert values == [1, 7, 100, 6, 5] and atoms == [1, 1, 1, 2, 2], (L, steps, atoms)
            assert ends == [(0, 0), (0, 0), (0, 0), (0, 0), (-1 << F, 0)]


def test_error_table(renderer):
    r = renderer
    F, L, n = 1014, 32, 4
    cx, cy = exact._to_limbs([0, 1, 2, 3], L), exact._to_limbs([0, 0, 0, 0], L)
    ln = np.array([5, 6, 7, 8], np.uint64)
    out = {k: np.zeros(n, np.uint64) for k in ("v", "a")}
    ex, ey = np.zeros((L, n), np.uint32), np.zeros((L, n), np.uint32)

    def raw(F=F, L=L, cx=cx, cy=cy, ln=ln, n=n, R=4, v=out["v"], a=out["a"], ex=ex, ey=ey):
        p = lambda x: None if x is None else x.ctypes.data
        return r._lib.fs_exact_eval_points_wide(r._h, F, L, p(cx), p(cy), p(ln), n, R, 0, p(v), p(a), p(ex), p(ey))

    assert raw() == 0 and list(out["v"]) == [5, 6, 7, 8]
    assert raw(n=0) == 0 and raw(n=0, cx=None, ln=None) == 0
    wide_cx = exact._to_limbs([0, 1, 2, 3], 705)
    for bad in (dict(L=1), dict(L=705, cx=wide_cx, cy=wide_cx), dict(F=1015), dict(R=0), dict(R=257)):
        assert raw(**bad) == FS_ERR_UNSUPPORTED, sorted(bad)
    for name in ("cx", "cy", "ln", "v", "a", "ex", "ey"):
        assert raw(**{name: None}) == INVALID, name
    assert raw(ln=np.array([5, 0, 7, 8], np.uint64)) == INVALID
    assert raw(ln=np.array([5, 6, 7, 2 ** 64 - 1], np.uint64)) == INVALID
    assert raw(n=2 ** 31) == INVALID
    assert raw(cx=exact._to_limbs([0, 1, 32 << F, 3], L)) == FS_ERR_UNSUPPORTED
    assert raw(cy=exact._to_limbs([0, 1, (-32 << F) - 1, 3], L)) == FS_ERR_UNSUPPORTED
    assert raw(cx=exact._to_limbs([0, 1, (32 << F) - 1, -32 << F], L)) == 0
    with pytest.raises(ValueError):
        exact.eval_points(r, [0], [0], [1], exact.MAX_WIDE_FRAC_BITS + 1, wide=True)
    with pytest.raises(ValueError):  # (without the keyword the limit is where it was)
        exact.eval_points(r, [0], [0], [1], exact.MAX_FRAC_BITS + 1)
    assert exact.eval_points(r, [], [], [], F, wide=True) == ([], [], [])


def test_a_frame_before_the_call_is_untouched(renderer):
    """The period planes of a rendered frame, its iteration buffer and a kept set stay what they were across a wide call, and the
    lane entry point still refuses 25 limbs behind it."""
    r, F = renderer, 246
    v = inputs.View("-2.2", "-1.2", "1.0", "1.2", 32, 24)
    v.num_iterations = 300
    assert r.InitializeMemory(v.width, v.height, 1, None, 0, 0, 0, False) == 0 and r.ClearMemory() == 0
    frame, atom = exact.render_periods(r, v, frac_bits=F)
    _check(r, 25, 4, False, "behind render_periods")
    err, atom2 = r.ExactAtomPeriods()
    assert err == 0 and np.array_equal(atom2.reshape(atom.shape), atom)
    exact.render(r, v, frac_bits=F, keep=True)
    kept = r.ExactKept()
    assert kept["valid"] == 1 and kept["samples"] > 0
    assert r.SetExactKeep(True) == 0 and r.SetExactPeriods(True) == 0 and r.SetExactCycleCheck(True) == 0  # (not read)
    _check(r, 25, 4, False, "behind a kept frame")
    assert r.SetExactKeep(False) == 0 and r.SetExactPeriods(False) == 0 and r.SetExactCycleCheck(False) == 0
    assert r.ExactKept() == kept
    out = r.new_iter_buffer()
    assert r.RenderCurrent(v.num_iterations, out) == 0 and r.SyncComputeStream() == 0
    assert np.array_equal(out[:v.height, :v.width], frame)
    exact.continue_render(r, 600)
    assert r.RenderCurrent(600, out) == 0 and r.SyncComputeStream() == 0
    raised = out[:v.height, :v.width].copy()
    assert r.DropExactKept() == 0
    exact.render(r, v, frac_bits=F, n_iterations=600)
    assert r.RenderCurrent(600, out) == 0 and r.SyncComputeStream() == 0
    assert np.array_equal(out[:v.height, :v.width], raised)
    L = 25
    z = exact._to_limbs([0], L)
    e = np.zeros((L, 1), np.uint32)
    one, o = np.array([1], np.uint64), np.zeros(1, np.uint64)
    assert r._lib.fs_exact_eval_points(r._h, 32 * L - 10, L, z.ctypes.data, z.ctypes.data, one.ctypes.data, 1, 4, 0, o.ctypes.data,
                                       o.ctypes.data, e.ctypes.data, e.ctypes.data) == FS_ERR_UNSUPPORTED


def test_statistics_of_a_small_call(renderer):
    """Three runs: c = 0 for 5 steps (v = 5), c = 1/4 for 9 (v = 9), c = 35/2 + i/3 which escapes at once (v = 0): 6 + 10 + 1 wave
    steps, 64 lane slots each, one launch."""
    r, L = renderer, 25
    F = 32 * L - 10
    values, atoms, ends = exact.eval_points(r, [0, model.fix(Fraction(1, 4), F), model.fix(Fraction(35, 2), F)],
                                            [0, 0, model.fix(Fraction(1, 3), F)], [5, 9, 40], F, wide=True)
    assert values == [5, 9, 0] and atoms == [1, 1, 0] and ends[2] is None and ends[0] == (0, 0)
    st = r.exact_stats()
    assert st == {"lane_slots": 64 * 17, "lane_steps": 17, "launches": 1, "running_after_first_slice": 0}
