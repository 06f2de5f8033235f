"""The exact renderer's period planes (fs_set_exact_periods; exact.render_periods) on the GPU.  Truth for both planes is the
definition restated on Python integers (tests/_atom_model.py), as recorded by tests/golden/make_exact_atom_model.py on these very
axes (tests/test_exact_atom_cpu.py runs the model again on a part of every record): the atom period looks at n and the norm only,
the cycle length at n only, so both are exact numbers whatever the cycle check, the slices and the compaction do.  The frame is the
switch-off frame byte for byte."""
import numpy as np
import pytest

import _atom_model as model
import _cycle_model as cycle
import _truth
from fractalshark_amd import GPURenderer, exact, inputs

pytestmark = pytest.mark.gpu

FS_ERR_6, FS_ERR_UNSUPPORTED = 10005, 10100
W, H, CAP = 64, 48, 20000  # the view and the cap of tests/test_gpu_exact_cycle.py


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


def _view(w=W, h=H, cap=CAP):
    v = inputs.View("-2.2", "-1.2", "1.0", "1.2", w, h)
    v.num_iterations = cap
    return v


_models = {}


def _model(v, F, R=4, inclusive=False):
    """(value, atom, cyclen) int64[H, W] of the view's frame, once per configuration: the record where there is one, else the model
    run here (small frames only)."""
    key = (tuple(v.bbox()), v.width, v.height, v.num_iterations, F, R, inclusive)
    if key not in _models:
        cx, cy = exact.axes(v, F)
        cap = v.num_iterations
        rec = model.recorded(model.record_key(v.width, v.height, F, R, inclusive, cap), cycle.axes_crc(cx, cy))
        if rec is None:
            assert v.width * v.height * cap <= 1 << 16, "no record for a frame this large: tests/golden/make_exact_atom_model.py"
            m = model.frame(cycle.from_limbs(cx), cycle.from_limbs(cy), F, R, inclusive, cap)
            rec = (m.value, m.atom, m.cyclen)
        _models[key] = tuple(a.reshape(v.height, v.width) for a in rec)
    return _models[key]


def _init(r, v, iter_bytes=4):
    assert r.InitializeMemory(v.width, v.height, 1, None, 0, 0, 0, False, iter_bytes=iter_bytes) == 0
    assert r.ClearMemory() == 0


def _plain(r, v, F, R=4, inclusive=False, iter_bytes=4, prove=False):
    """The switch-off frame of exact.render."""
    _init(r, v, iter_bytes)
    exact.render(r, v, bailout=R, frac_bits=F, iter_bytes=iter_bytes, inclusive=inclusive, prove_interior=prove)
    out = r.new_iter_buffer()
    assert r.RenderCurrent(v.num_iterations, out) == 0 and r.SyncComputeStream() == 0
    return out[:v.height, :v.width].copy()


def _periods(r, v, F, R=4, inclusive=False, iter_bytes=4, prove=False):
    _init(r, v, iter_bytes)
    return exact.render_periods(r, v, bailout=R, frac_bits=F, iter_bytes=iter_bytes, inclusive=inclusive, prove_interior=prove)


def _check(v, F, R, inclusive, off_frame, got, prove, what):
    """One render_periods result against the switch-off frame and the model."""
    value, atom, cyclen = _model(v, F, R, inclusive)
    assert len(got) == (3 if prove else 2)
    frame, a = got[0], got[1]
    assert frame.dtype == off_frame.dtype and frame.tobytes() == off_frame.tobytes(), what
    assert np.array_equal(frame.astype(np.int64), value), what
    assert a.dtype == np.uint64 and a.shape == frame.shape
    bad = int((a.astype(np.int64) != atom).sum())
    print("atom %-40s %d pixels, %d atom periods, %d differ from the model" % (what, a.size, len(np.unique(atom)), bad))
    assert bad == 0, what
    if prove:
        lam = got[2]
        assert lam.dtype == np.uint64 and np.array_equal(lam.astype(np.int64), cyclen), what


@pytest.mark.parametrize("F,R,inclusive,iter_bytes", [(54, 4, False, 4), (246, 4, False, 4), (758, 4, False, 4), (246, 256, False, 4),
                                                      (246, 4, True, 4), (246, 4, False, 8)])
def test_frame_and_planes(renderer, F, R, inclusive, iter_bytes):
    assert exact.limbs_for(F) == {54: 2, 246: 8, 758: 24}[F]
    r, v = renderer, _view()
    value, atom, cyclen = _model(v, F, R, inclusive)
    assert (int((atom == 0).sum()) > 0) == (R == 4) and len(np.unique(atom)) > 20 and int((cyclen != 0).sum()) > 500
    off_frame = _plain(r, v, F, R, inclusive, iter_bytes)
    what = "F %d R %d incl %d ib %d" % (F, R, inclusive, iter_bytes)
    got = _periods(r, v, F, R, inclusive, iter_bytes)
    _check(v, F, R, inclusive, off_frame, got, False, what)
    assert r.ExactCycleLengths()[0] == FS_ERR_6  # the cycle check was off
    # with the cycle check: the atom plane unchanged, the cycle lengths the model's, non-zero exactly on the proved mask
    on = _periods(r, v, F, R, inclusive, iter_bytes, prove=True)
    _check(v, F, R, inclusive, off_frame, on, True, what + " proving")
    assert on[1].tobytes() == got[1].tobytes()
    err, proved = r.ExactProved()
    assert err == 0 and np.array_equal(proved.reshape(H, W) != 0, on[2] != 0) and int(proved.sum()) > 500


def test_slices_and_compaction(renderer):
    """State per pixel, reloaded at the start of every slice: slices of 16 steps with and without compaction, and of 1000, with the
    cycle check off (every sample to the cap: interior pixels walk their cycle and meet their smallest norm again and again, which
    the full compare must answer with "not less") and on."""
    r, F = renderer, 246
    v = _view()
    off_frame = _plain(r, v, F)
    for prove in (False, True):
        for steps, loose in ((16, False), (16, True), (1000, False)):
            assert r.SetExactSlice(steps, no_compaction=loose) == 0
            got = _periods(r, v, F, prove=prove)
            _check(v, F, 4, False, off_frame, got, prove, "F 246 slice %d%s%s" % (steps, " no compaction" if loose else "",
                                                                               " proving" if prove else ""))


def test_narrow_keys(renderer):
    """With a key of 6 bits -- the index of the highest limb that is not zero -- nearly every step reads the minimum back and the
    full compare decides; with 40 bits, many do.  No plane changes."""
    r, F = renderer, 246
    v = _view()
    off_frame = _plain(r, v, F)
    for bits in (6, 40):
        assert r.SetExactAtomKeyBits(bits) == 0
        _check(v, F, 4, False, off_frame, _periods(r, v, F, prove=True), True, "F 246 key of %d bits" % bits)
    assert r.SetExactSlice(100) == 0
    _check(v, F, 4, False, off_frame, _periods(r, v, F), False, "F 246 key of 40 bits, slice 100")


def test_fixture_frame(renderer):
    """70 x 37 = 2590 samples: the list does not fill its last wave."""
    c = _truth.Case("view0_70x37")
    v, F = c.view(inputs), c.raw["frac_bits"]
    v.num_iterations = c.cap
    assert (v.width, v.height) == (c.w, c.h) == (70, 37) and (c.w * c.h) % 64 != 0
    off_frame = _plain(renderer, v, F)
    for prove in (False, True):
        _check(v, F, 4, False, off_frame, _periods(renderer, v, F, prove=prove), prove, "view0_70x37%s" % (" proving" if prove else ""))


def test_every_take_on_a_slice_boundary(renderer):
    """8 x 8 at cap 64 with slices of one step: every take is the only step of its launch, and the key comes from memory each time."""
    r, F = renderer, 54
    v = _view(8, 8, 64)
    off_frame = _plain(r, v, F)
    assert r.SetExactSlice(1) == 0
    for prove in (False, True):
        got = _periods(r, v, F, prove=prove)
        _check(v, F, 4, False, off_frame, got, prove, "8 x 8, slices of 1%s" % (" proving" if prove else ""))
    assert len(np.unique(_model(v, F)[1])) > 3


def test_switch_semantics(native_libs):
    fresh = GPURenderer(0)
    try:
        r, F = fresh, 54
        v = _view(16, 12, 500)
        n = 16 * 12
        assert r.ExactAtomPeriods(n)[0] == FS_ERR_6 and r.ExactCycleLengths(n)[0] == FS_ERR_6  # nothing rendered yet
        off_frame = _plain(r, v, F, prove=True)  # off by default
        assert r.ExactAtomPeriods()[0] == FS_ERR_6 and r.ExactCycleLengths()[0] == FS_ERR_6
        st_off = r.exact_stats()
        got = _periods(r, v, F)
        assert got[0].tobytes() == off_frame.tobytes()
        assert r.ExactAtomPeriods()[0] == 0 and r.ExactCycleLengths()[0] == FS_ERR_6  # the cycle check was off
        assert r.ExactAtomPeriods(5)[0] == 1  # hipErrorInvalidValue: not the plane's size
        on = _periods(r, v, F, prove=True)
        assert r.ExactCycleLengths()[0] == 0 and on[1].tobytes() == got[1].tobytes() and r.exact_stats() == st_off
        # render_periods has switched the planes off again behind itself: a plain render invalidates both readers
        again = _plain(r, v, F, prove=True)
        assert again.tobytes() == off_frame.tobytes()
        assert r.ExactAtomPeriods()[0] == FS_ERR_6 and r.ExactCycleLengths()[0] == FS_ERR_6

        # the switch and keep together: refused before the frame or the kept set is touched
        exact.render(r, v, bailout=4, frac_bits=F, keep=True)
        kept = r.ExactKept()
        assert kept["valid"] and kept["samples"] > 0
        marked = _plain_read(r, v)
        assert r.SetExactPeriods(True) == 0 and r.SetExactKeep(True) == 0
        cx, cy = exact.axes(v, F)
        assert r.RenderExact(4, F, exact.limbs_for(F), cx, cy, 4, False, 77) == FS_ERR_UNSUPPORTED
        assert r.ExactKept() == kept and _plain_read(r, v).tobytes() == marked.tobytes()
        assert r.SetExactKeep(False) == 0
        # the continuation ignores the switch (still on), and leaves the readers as they were
        assert exact.continue_render(r, 600) is None
        assert r.ExactAtomPeriods()[0] == FS_ERR_6
        assert r.SetExactPeriods(False) == 0
        v600 = _view(16, 12, 600)
        assert _plain_read(r, v600).tobytes() == _plain(r, v600, F).tobytes()
    finally:
        fresh.close()


def _plain_read(r, v):
    out = r.new_iter_buffer()
    assert r.RenderCurrent(v.num_iterations, out) == 0 and r.SyncComputeStream() == 0
    return out[:v.height, :v.width].copy()


def test_other_entry_points_ignore_the_switch(renderer):
    """stable_mask, the audit and the wide path: the same results with the switch on as with it off, and the planes of the last
    fs_render_exact stay readable."""
    r = renderer
    v = _view()
    F = v.precision_bits + exact.GUARD_BITS
    _init(r, v)
    frame, atom = exact.render_periods(r, v, frac_bits=F)
    xs, ys = exact.lattice(v, 8, 6)

    def others():
        mask = exact.stable_mask(r, v, 12)
        st_mask = r.exact_stats()
        rep = exact.audit(r, v, xs, ys, levels=(10,), bailout=4)
        return mask, st_mask, bytes(rep.record), rep.values.copy(), r.exact_stats()

    off = others()
    assert r.SetExactPeriods(True) == 0
    on = others()
    assert np.array_equal(on[0], off[0]) and on[1] == off[1] and on[2] == off[2] and np.array_equal(on[3], off[3]) and on[4] == off[4]
    err, kept_atom = r.ExactAtomPeriods()
    assert err == 0 and np.array_equal(kept_atom.reshape(H, W), atom)

    # the wide path
    vb = _truth.boundary_view(inputs)
    n, cap, Fw, L = _truth.BOUNDARY_SIZE, _truth.BOUNDARY_CAP, 790, 25
    assert exact.uses_wide(L)
    cx, cy = exact.axes(vb, Fw, limbs=L)
    assert r.InitializeMemory(n, n, 1, None, 0, 0, 0, False) == 0

    def wide():
        assert r.ClearMemory() == 0
        assert r.RenderExactWide(4, Fw, L, cx, cy, 4, False, cap) == 0
        out = r.new_iter_buffer()
        assert r.RenderCurrent(cap, out) == 0 and r.SyncComputeStream() == 0
        return out[:n, :n].copy(), r.exact_stats()

    with_switch = wide()
    assert r.SetExactPeriods(False) == 0
    without = wide()
    assert with_switch[0].tobytes() == without[0].tobytes() and with_switch[1] == without[1]
    with pytest.raises(ValueError):
        exact.render_periods(r, vb, frac_bits=Fw)
