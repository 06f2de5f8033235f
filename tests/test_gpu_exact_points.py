"""Point runs on the GPU (fs_exact_eval_points; exact.eval_points): values, atom periods and every limb of every endpoint against the
definitions on Python integers (tests/_point_model.py).  No tolerance anywhere: the device evaluates the exact recurrence."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import _point_model as model
from fractalshark_amd import GPURenderer, exact, inputs

pytestmark = pytest.mark.gpu

FS_ERR_UNSUPPORTED, INVALID = 10100, 1  # (hipErrorInvalidValue)
LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 100, 333, 1000)  # (15 .. 33 straddle the ends of slices of 16)
POINTS = [(0, 0), (-1, 0), (Fraction(1, 4), 0), (Fraction(5, 2), Fraction(1, 3)), (-2, 0), (Fraction(-3, 4), Fraction(1, 20)),
          (Fraction(-12253, 100000), Fraction(74484, 100000)), (Fraction(35, 2), Fraction(1, 3)), (Fraction(-1, 2), Fraction(1, 2)),
          (Fraction(3, 10), Fraction(1, 2)), (Fraction(-7, 4), Fraction(1, 1000)), (Fraction(-3, 4), Fraction(1, 100)),
          (Fraction(28, 100), Fraction(1, 100))]
N_RUNS = 130  # two full waves and two lanes of a third


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _switches_off(renderer):
    yield
    assert renderer.SetExactPeriods(False) == 0 and renderer.SetExactAtomKeyBits(0) == 0
    assert renderer.SetExactCycleCheck(False) == 0 and renderer.SetExactKeep(False) == 0
    assert renderer.SetExactSlice(0) == 0


def _runs(F, n=N_RUNS, lengths=LENGTHS):
    """n runs: the points in turn, the lengths in turn (13 points, 14 lengths: every pair comes up over 182 runs)."""
    cxs = [model.fix(POINTS[k % len(POINTS)][0], F) for k in range(n)]
    cys = [model.fix(POINTS[k % len(POINTS)][1], F) for k in range(n)]
    return cxs, cys, [lengths[k % len(lengths)] for k in range(n)]


_models = {}


def _model(F, R, inclusive, n=N_RUNS, lengths=LENGTHS):
    """The model on _runs, once per configuration, never changed."""
    key = (F, R, inclusive, n, lengths)
    if key not in _models:
        cxs, cys, ps = _runs(F, n, lengths)
        _models[key] = [model.run(a, b, F, R, inclusive, p) for a, b, p in zip(cxs, cys, ps)]
    return _models[key]


def _check(r, F, R, inclusive, what, n=N_RUNS, lengths=LENGTHS):
    cxs, cys, ps = _runs(F, n, lengths)
    want = _model(F, R, inclusive, n, lengths)
    values, atoms, ends = exact.eval_points(r, cxs, cys, ps, F, bailout=R, inclusive=inclusive)
    bad = [k for k in range(n) if (values[k], atoms[k], ends[k]) != want[k]]
    print("points %-44s %d runs, %d short of their length, %d differ from the model" % (what, n, sum(1 for w in want if w[2] is None),
                                                                                      len(bad)))
    assert not bad, (what, bad[:4], [(values[k], atoms[k], ends[k], want[k]) for k in bad[:2]])
    st = r.exact_stats()
    assert st["lane_steps"] == sum(w[0] + 1 for w in want) and st["launches"] >= 1, (what, st)  # a run makes v + 1 escape tests
    return st


@pytest.mark.parametrize("F", [54, 246, 758])
@pytest.mark.parametrize("R,inclusive", [(4, False), (256, False), (4, True), (256, True)])
def test_runs_equal_the_model(renderer, F, R, inclusive):
    """130 runs in one call (a last wave that is not full), lengths 1 .. 1000 mixed, runs that escape before, at and after their
    length among runs that do not; 2, 8 and 24 limbs."""
    assert exact.limbs_for(F) == {54: 2, 246: 8, 758: 24}[F]
    want = _model(F, R, inclusive)
    short = sum(1 for w in want if w[2] is None)
    assert 10 < short < N_RUNS - 40 and len({w[1] for w in want}) > 8
    assert any(w[2] is None and 0 < w[0] for w in want) and (R != 4 or any(w[0] == 0 for w in want))
    _check(renderer, F, R, inclusive, "F %d R %d incl %d" % (F, R, inclusive))
    # the raw call: the endpoint planes of a run short of its length are zero on every limb
    L = exact.limbs_for(F)
    cxs, cys, ps = _runs(F)
    err, values, atoms, end_x, end_y = renderer.ExactEvalPoints(F, L, exact._to_limbs(cxs, L), exact._to_limbs(cys, L),
                                                                np.array(ps, np.uint64), R, inclusive)
    assert err == 0 and end_x.shape == end_y.shape == (L, N_RUNS)
    for k, w in enumerate(want):
        if w[2] is None:
            assert not end_x[:, k].any() and not end_y[:, k].any(), k


def test_slices_and_compaction(renderer):
    """Slices of 16 with and without compaction, and of 1: runs whose lengths straddle a slice end leave the list at different
    slices; the per-run state is reloaded at the start of every slice."""
    r, F = renderer, 246
    base = _check(r, F, 4, False, "default slice")
    for steps, fixed in ((16, False), (16, True)):
        assert r.SetExactSlice(steps, fixed) == 0
        st = _check(r, F, 4, False, "slice %d%s" % (steps, " fixed slots" if fixed else ""))
        assert st["launches"] == (1000 + 1 + 15) // 16 and st["lane_steps"] == base["lane_steps"]
    assert r.SetExactSlice(1, False) == 0
    short = tuple(p for p in LENGTHS if p <= 65)
    st = _check(r, F, 4, False, "slice 1", lengths=short)
    assert st["launches"] == 66
    assert r.SetExactSlice(16, False) == 0
    _check(r, 54, 256, True, "slice 16, 2 limbs, inclusive")
    _check(r, 758, 4, False, "slice 16, 24 limbs")


@pytest.mark.parametrize("bits", [6, 40])
def test_narrow_keys(renderer, bits):
    """The point-run kernels honour fs_set_exact_atom_key_bits: with the narrowest key nearly every tracked state reads the run's
    minimum back and compares all limbs; the results do not move."""
    r = renderer
    assert r.SetExactAtomKeyBits(bits) == 0 and r.SetExactSlice(16, False) == 0
    _check(r, 246, 4, False, "key %d bits" % bits)
    _check(r, 758, 256, False, "key %d bits, 24 limbs" % bits)


def test_switches_are_ignored(renderer):
    r = renderer
    assert r.SetExactCycleCheck(True) == 0 and r.SetExactKeep(True) == 0 and r.SetExactPeriods(True) == 0
    _check(r, 246, 4, False, "cycle check, keep and periods on")
    assert r.ExactKept()["valid"] == 0 and r.ExactAtomPeriods(N_RUNS)[0] != 0 and r.ExactProved(N_RUNS)[0] != 0


def test_fixture_points_at_the_views_precision(renderer):
    """The 86 found points of the View 5 fixture as printed, at F = 331, each with its own period as its length, in one call; the
    model on every fifth.  What the issue found on them: point 0 (period 79 420) has its smallest norm at n = 16 045; point 43
    (period 16 045) is the one whose atom period is its period."""
    F = 331
    found = model.fixture()
    starts = [model.fixture_point(pt, F) for pt in found]
    cxs, cys, ps = [s[0][0] for s in starts], [s[0][1] for s in starts], [s[2] for s in starts]
    values, atoms, ends = exact.eval_points(renderer, cxs, cys, ps, F)
    for k in range(0, len(found), 5):
        assert (values[k], atoms[k], ends[k]) == model.run(cxs[k], cys[k], F, 256, False, ps[k]), k
    assert (ps[0], values[0], atoms[0]) == (79420, 79420, 16045) and (ps[43], values[43], atoms[43]) == (16045, 16045, 16045)
    assert all((e is None) == (v < p) for e, v, p in zip(ends, values, ps)) and all(a <= v for a, v in zip(atoms, values))
    print("fixture at F 331: %d of 86 runs reach their period, %d of them with atom period == period" % (
        sum(1 for e in ends if e is not None), sum(1 for a, p, e in zip(atoms, ps, ends) if e is not None and a == p)))


def test_error_table(renderer):
    r = renderer
    F, L, n = 246, 8, 4
    cx, cy = exact._to_limbs([0, 1, 2, 3], L), exact._to_limbs([0, 0, 0, 0], L)
    ln = np.array([5, 6, 7, 8], np.uint64)
    out = {k: np.zeros(n, np.uint64) for k in ("v", "a")}
    ex, ey = np.zeros((L, n), np.uint32), np.zeros((L, n), np.uint32)

    def raw(F=F, L=L, cx=cx, cy=cy, ln=ln, n=n, R=4, v=out["v"], a=out["a"], ex=ex, ey=ey):
        p = lambda x: None if x is None else x.ctypes.data
        return r._lib.fs_exact_eval_points(r._h, F, L, p(cx), p(cy), p(ln), n, R, 0, p(v), p(a), p(ex), p(ey))

    assert raw() == 0 and list(out["v"]) == [5, 6, 7, 8]
    assert raw(n=0) == 0 and raw(n=0, cx=None, ln=None) == 0
    for bad in (dict(L=1), dict(L=25), dict(F=247), dict(R=0), dict(R=257)):
        assert raw(**bad) == FS_ERR_UNSUPPORTED, bad
    for name in ("cx", "cy", "ln", "v", "a", "ex", "ey"):
        assert raw(**{name: None}) == INVALID, name
    assert raw(ln=np.array([5, 0, 7, 8], np.uint64)) == INVALID
    assert raw(ln=np.array([5, 6, 7, 2 ** 64 - 1], np.uint64)) == INVALID
    assert raw(n=2 ** 31) == INVALID
    assert raw(cx=exact._to_limbs([0, 1, 32 << F, 3], L)) == FS_ERR_UNSUPPORTED
    assert raw(cy=exact._to_limbs([0, 1, (-32 << F) - 1, 3], L)) == FS_ERR_UNSUPPORTED
    assert raw(cx=exact._to_limbs([0, 1, (32 << F) - 1, -32 << F], L)) == 0
    with pytest.raises(ValueError):
        exact.eval_points(r, [0], [0], [1], exact.MAX_FRAC_BITS + 1)
    assert exact.eval_points(r, [], [], [], F) == ([], [], [])


def test_a_frame_before_the_call_is_untouched(renderer):
    """The period planes of a rendered frame, its iteration buffer and a kept set stay what they were across a call."""
    r, F = renderer, 246
    v = inputs.View("-2.2", "-1.2", "1.0", "1.2", 32, 24)
    v.num_iterations = 300
    assert r.InitializeMemory(v.width, v.height, 1, None, 0, 0, 0, False) == 0 and r.ClearMemory() == 0
    frame, atom = exact.render_periods(r, v, frac_bits=F)
    _check(r, F, 4, False, "behind render_periods")
    err, atom2 = r.ExactAtomPeriods()
    assert err == 0 and np.array_equal(atom2.reshape(atom.shape), atom)
    exact.render(r, v, frac_bits=F, keep=True)
    kept = r.ExactKept()
    assert kept["valid"] == 1 and kept["samples"] > 0
    _check(r, F, 4, False, "behind a kept frame")
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
