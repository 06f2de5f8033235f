"""GPU: the BLA tables on the device -- the builder, the three texts of the lookup, and the derived tables of the default kernel --
against the host builder and the plain model of tests/_bla_model.py (pinned on the CPU by tests/test_bla_model_cpu.py).  Every
comparison is equality of bits or bytes.

  1. fs_build_bla against the host builder at every M of the case set (orbits of M + 1 entries of Views 19 and 5: tiny ones, powers
     of two and one past them, 4099 = ragged at every level), HDRFloat<float> and <double>, padding included; the tables in which
     no lookup can apply (M <= 4) render perturbation-only; one table with a bla_size that is not the orbit's own.
  2. bla_lookup<float>, bla_lookup<double> and bla_lookup_native asked directly (fs_bla_lookup_probe) at every orbit index, at the
     keys on both sides of every r2 their walk meets, on built and on uploaded tables.
  3. The derived tables read back (fs_read_bla_native): native records, ladder, pre-test keys, heap records, heap ladder, Q and zb
     byte for byte against the model, and the model's walks over the tables that were read back.
  4. Frames through all three kernels (heap, compiled on the native form, literal on the reference layout) at three caps, and the
     staleness of the native form when the orbit or the table is replaced under it.

Poison classes the byte comparison covers (counted on the CPU by test_poison_classes_of_the_derived_tables_are_reached): a jump that
would leave the orbit (l = 0xFFFFFFFF), an arrival at the orbit's last entry, arrival entries above 2^1 and below 2^-40
(Orbit.scale_entries), a coefficient exponent at or below -2^26 (exact zeros), Q entries of level 0, the three kinds of zb entry.
Not reachable by any orbit: a coefficient mantissa beyond 2^30 -- the coefficients of levels 2 and up are reduced results of a
merge, or an orbit mantissa times one, or the constants 1 and 0; the orbit edits move exponents only."""
import numpy as np
import pytest

import _bla_model as bm
import _oracle
from fractalshark_amd import GPURenderer, T_HDR32, T_HDR64

pytestmark = pytest.mark.gpu

W, H = 70, 37
LOOKUP_M = [M for M in bm.M_SET if M >= 3]       # tables of more than two levels: the lookups can be asked
FRAME_M = (5, 9, 17, 33, 257, 1025, 4099)
# (heap_height: a table whose only level-2-and-up record is the one of level 2 has H = 2, below the 3 the heap needs)
NO_HEAP_M = (3, 4)


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    assert r.InitializeMemory(W, H, 1, None, 0, 0, 0, False) == 0
    yield r
    r.set_kernel_variant(0)
    r.close()


def _upload_orbit(r, c):
    T = T_HDR64 if c.is64 else T_HDR32
    assert r._lib.fs_upload_orbit(r._h, 0, T, 4, c.orbit.data_ptr, c.orbit.count, c.orbit.count, c.orbit.period) == 0
    return T


def _install(r, c, built):
    """The case's orbit, then its table: built on the device from that orbit, or the host builder's uploaded."""
    T = _upload_orbit(r, c)
    if built:
        assert r.BuildBLAOnDevice(c.orbit, bla_size=c.bla_size) == 0
    else:
        assert r._lib.fs_upload_bla(r._h, T, c.bla.level_ptrs, c.bla.level_sizes, c.bla.num_levels, c.bla.lm2) == 0
    return T


def _render(r, c, T, n, variant=0):
    co = c.view.coords_perturb(c.orbit)
    assert r.set_kernel_variant(variant) == 0
    try:
        assert r.ClearMemory() == 0
        assert r._lib.fs_render_bla(r._h, T, co.ctypes.data, n) == 0
        buf = r.new_iter_buffer()
        assert r.RenderCurrent(n, buf) == 0
        assert r.SyncComputeStream() == 0
    finally:
        r.set_kernel_variant(0)
    return buf


def _assert_table_equals_host(r, c):
    assert r._lib.fs_bla_num_levels(r._h) == c.bla.num_levels and r._lib.fs_bla_lm2(r._h) == c.bla.lm2
    dev = r.read_bla_levels(c.is64)
    assert [len(a) for a in dev] == c.bla.sizes()
    for l, a in enumerate(dev):
        assert a.tobytes() == c.tab.raw[l].tobytes(), "level %d differs" % l


# ---------------------------------------------------------------------------------------------- 1. the builder
@pytest.mark.parametrize("is64", [False, True])
@pytest.mark.parametrize("M", bm.M_SET)
def test_table_built_on_device_equals_host_builder(renderer, native_libs, M, is64):
    r = renderer
    for view_n in (19, 5):
        c = bm.case(view_n, M, is64)
        T = _install(r, c, built=True)
        _assert_table_equals_host(r, c)
        if M > 4:
            continue
        # no lookup can apply: nothing materialised (M = 1, 2), or one record of level 2 under lm2 = 1 (M = 3, 4).  The frame is the
        # perturbation-only one.  (The reference's lookup reads the first record of level 2 at m = 1: it cannot be handed a table
        # of one or two levels, so the oracle of M = 1, 2 runs without one -- which is what "no lookup applies" means.)
        assert c.bla.num_levels == (M if M < 3 else 3) and c.bla.lm2 == (0 if M < 3 else 1)
        out = _render(r, c, T, 1000)
        assert np.array_equal(out, _oracle.bla_hdr32(c.view, c.orbit, c.bla if M >= 3 else None, n_iterations=1000)), (view_n, M)
        assert np.array_equal(out, _oracle.bla_hdr32(c.view, c.orbit, None, n_iterations=1000)), (view_n, M)


@pytest.mark.parametrize("is64", [False, True])
def test_table_built_with_another_bla_size(renderer, native_libs, is64):
    """BLAS::Init's blaSize is an argument of its own: the orbit's max_radius() scaled by 2^-20, on both sides (on the shallow view, where
    the term it enters is not negligible: six of eight levels change)."""
    c, c0 = bm.case("shallow", 257, is64, None, -20), bm.case("shallow", 257, is64)
    assert any(c.tab.raw[l].tobytes() != c0.tab.raw[l].tobytes() for l in range(2, c.tab.n_levels))
    T = _install(renderer, c, built=True)
    _assert_table_equals_host(renderer, c)
    assert np.array_equal(_render(renderer, c, T, 1000), _oracle.bla_hdr32(c.view, c.orbit, c.bla, n_iterations=1000))


# ---------------------------------------------------------------------------------------------- 2. the three lookups
@pytest.mark.parametrize("built", [True, False], ids=["built", "uploaded"])
@pytest.mark.parametrize("M", LOOKUP_M)
def test_three_lookups_answer_every_question_as_the_model(renderer, native_libs, M, built):
    r = renderer
    for view_n in (19, 5):
        c = bm.case(view_n, M, False)
        m, z2 = bm.pack_questions(c.questions, False)
        _install(r, c, built)
        assert np.array_equal(r.bla_lookup_probe(0, m, z2), c.answers), ("bla_lookup<float>", view_n, M)
        assert np.array_equal(r.bla_lookup_probe(2, m, z2), c.answers), ("bla_lookup_native", view_n, M)
        c = bm.case(view_n, M, True)
        m, z2 = bm.pack_questions(c.questions, True)
        _install(r, c, built)
        assert np.array_equal(r.bla_lookup_probe(1, m, z2), c.answers), ("bla_lookup<double>", view_n, M)


# ---------------------------------------------------------------------------------------------- 3. the derived tables
def _derived_cases():
    return [(19, M, None) for M in LOOKUP_M] + [(5, M, None) for M in (5, 33, 1025)] + [(19, M, "window") for M in (17, 65, 257)]


@pytest.mark.parametrize("view_n,M,edit", _derived_cases())
@pytest.mark.parametrize("built", [True, False], ids=["built", "uploaded"])
def test_derived_tables_equal_the_model_byte_for_byte(renderer, native_libs, view_n, M, edit, built):
    _check_derived(renderer, bm.case(view_n, M, False, edit), built)


@pytest.mark.parametrize("M", [33, 1025])
def test_uploaded_table_in_which_the_gate_of_the_first_index_decides(renderer, native_libs, M):
    """A builder's table cannot show whether Q[0] carries the gate of BLAS.cpp:270-281: there the r2 of (2, 0) is the largest the
    walk at m = 1 meets, and the pre-test key alone equals it.  An uploaded table is whatever the host hands over: this one has
    larger r2 above (2, 0), so that z2 between the two passes every probe of the walk and only the gate says no."""
    r = renderer
    c = bm.case(19, M, False, "wide_first")
    assert c.tab.r2[3][0] > c.tab.r2[2][0] and int(c.derived.q["key"][0]) < int(c.derived.pretest[0])
    _check_derived(r, c, built=False)
    m, z2 = bm.pack_questions(c.questions, False)
    assert np.array_equal(r.bla_lookup_probe(0, m, z2), c.answers)
    assert np.array_equal(r.bla_lookup_probe(2, m, z2), c.answers)
    ref = _oracle.bla_hdr32(c.view, c.orbit, c.bla, n_iterations=1000)
    T = T_HDR32
    for variant in (0, 2, 1):
        assert np.array_equal(_render(r, c, T, 1000, variant), ref), variant


def _check_derived(r, c, built):
    view_n, M, edit = c.view_n, c.M, None
    d = c.derived
    _install(r, c, built)
    g = r.read_bla_native()
    assert g["native_ok"] and not d.bad
    assert (g["n_levels"], g["lm2"], g["total"], g["orbit_count"], g["n_q"]) == (d.tab.n_levels, d.tab.lm2, d.total, d.count, d.n_q)
    assert g["level_off"][:d.tab.n_levels] == d.level_off and g["level_n"][:d.tab.n_levels] == d.level_n
    assert g["H"] == d.H and g["heap_positions"] == d.heap_positions and g["heap_ok"] == (d.H != 0)
    assert g["heap_ok"] == (M not in NO_HEAP_M)
    want = d.part_bytes()
    for name in GPURenderer.BLA_NATIVE_PARTS[1:]:
        assert (name in g) == (name in want), name
        if name in want:
            assert g[name].tobytes() == want[name], (name, view_n, M, edit)
    # the model's walks over the tables that were READ BACK answer the whole question set as the model's lookup does
    ladder = np.frombuffer(g["ladder"].tobytes(), np.int64).reshape(-1, 4)
    pretest = np.frombuffer(g["pretest"].tobytes(), np.int64)
    passed_pretest_and_missed = 0
    if g["heap_ok"]:
        q = np.frombuffer(g["q"].tobytes(), bm.Q_DTYPE)
        heap_ladder = np.frombuffer(g["heap_ladder"].tobytes(), np.int64).reshape(-1, 4)
    for (m, z), a in zip(c.questions, c.answers):
        want_a = tuple(int(x) for x in a) if a[0] != 0xFFFFFFFF else None
        zk = bm.zkey_of(z)
        p = bm.walk_native(ladder, pretest, g["level_off"], g["lm2"], m, zk)
        assert (None if p is None else bm.native_level_ix(g["level_off"], g["level_n"], p)) == want_a, (m, z)
        if bm.probes(g["lm2"], m) and want_a is None and (m != 1 or z < c.tab.r2[2][0]) and zk < int(pretest[(m - 1) >> 2]):
            passed_pretest_and_missed += 1
        if g["heap_ok"]:
            def slow(mm, kk):
                pp = bm.walk_native(ladder, pretest, g["level_off"], g["lm2"], mm, kk)
                return None if pp is None else bm.native_level_ix(g["level_off"], g["level_n"], pp)
            assert bm.walk_heap(q, heap_ladder, g["H"], m, zk, slow) == want_a, (m, z)
    assert passed_pretest_and_missed == 0  # (no pre-test key on the device is too large: tests/test_bla_model_cpu.py's docstring)


# ---------------------------------------------------------------------------------------------- 4. frames and staleness
_frame_refs = {}


def _frame_caps_and_refs(c):
    """Three caps -- 1, 1000, one above the longest count of the oracle's frame -- and the oracle's frames, computed once."""
    key = (c.view_n, c.M)
    if key not in _frame_refs:
        longest = int(_oracle.bla_hdr32(c.view, c.orbit, c.bla, n_iterations=20000)[:H, :W].max())
        _frame_refs[key] = {n: _oracle.bla_hdr32(c.view, c.orbit, c.bla, n_iterations=n) for n in (1, 1000, longest + 1)}
    return _frame_refs[key]


@pytest.mark.parametrize("built", [True, False], ids=["built", "uploaded"])
@pytest.mark.parametrize("M", (33, 257))
def test_frames_of_a_shallow_view_through_all_three_kernels(renderer, native_libs, M, built):
    """As below on a view whose pixels differ: 625 different counts in the frame, where View 19's frame under so short an orbit
    holds one."""
    r = renderer
    c = bm.case("shallow", M, False)
    T = _install(r, c, built)
    refs = _frame_caps_and_refs(c)
    assert len(np.unique(refs[max(refs)][:H, :W])) > 500
    for n, ref in refs.items():
        for variant in (0, 2, 1):
            assert np.array_equal(_render(r, c, T, n, variant), ref), (M, n, variant)


@pytest.mark.parametrize("built", [True, False], ids=["built", "uploaded"])
@pytest.mark.parametrize("M", FRAME_M)
def test_frames_through_all_three_kernels(renderer, native_libs, M, built):
    """variant 0: the hand-written kernel on the heap form; 2: the compiled kernel on the native form; 1: the literal kernel on
    the reference layout.  Every M here has a heap (H >= 3): none falls back to the compiled kernel by default -- the tables that do
    (NO_HEAP_M) have no lookup that applies and are rendered by test_table_built_on_device_equals_host_builder."""
    r = renderer
    c = bm.case(19, M, False)
    T = _install(r, c, built)
    g = r.read_bla_native()
    assert c.derived.H >= 3 and g["native_ok"] and g["heap_ok"] and g["H"] == c.derived.H
    for n, ref in _frame_caps_and_refs(c).items():
        for variant in (0, 2, 1):
            assert np.array_equal(_render(r, c, T, n, variant), ref), (M, n, variant)


@pytest.mark.parametrize("M", NO_HEAP_M)
def test_without_a_heap_the_default_is_the_compiled_kernel(renderer, native_libs, M):
    r = renderer
    c = bm.case(19, M, False)
    for built in (True, False):
        T = _install(r, c, built)
        g = r.read_bla_native()
        assert g["native_ok"] and not g["heap_ok"] and g["H"] == 0
        ref = _oracle.bla_hdr32(c.view, c.orbit, c.bla, n_iterations=1000)
        for variant in (0, 2, 1):
            assert np.array_equal(_render(r, c, T, 1000, variant), ref), (M, variant)


def _fresh_frame(native_libs, c, n, built):
    r = GPURenderer(0)
    try:
        assert r.InitializeMemory(W, H, 1, None, 0, 0, 0, False) == 0
        T = _install(r, c, built)
        return _render(r, c, T, n)
    finally:
        r.close()


def test_native_form_follows_a_new_orbit_and_a_new_table(renderer, native_libs):
    """The native form carries arrival entries of the orbit and keys of the table it was made from: whichever of the two is
    replaced, the next frame is the frame of a fresh renderer given only the final inputs (and the oracle's)."""
    r = renderer
    n = 1000
    a, b = bm.case(19, 257, False), bm.case(5, 257, False)   # two orbits of one length
    assert a.orbit.count == b.orbit.count and a.orbit.entries().tobytes() != b.orbit.entries().tobytes()
    ref_b = _oracle.bla_hdr32(b.view, b.orbit, b.bla, n_iterations=n)
    # table A with orbit A rendered, then orbit B uploaded, then table B built from it
    T = _install(r, a, built=False)
    assert np.array_equal(_render(r, a, T, n), _oracle.bla_hdr32(a.view, a.orbit, a.bla, n_iterations=n))
    _upload_orbit(r, b)
    # (the native form of table A is stale from here on: read back, it is table A's keys with orbit B's arrival entries)
    g = r.read_bla_native()
    mixed = bm.Derived(a.tab, b.orbit.entries())
    assert g["records"].tobytes() == mixed.records.tobytes() and g["zb"].tobytes() == mixed.zb.tobytes()
    assert g["records"].tobytes() != a.derived.records.tobytes()
    assert r.BuildBLAOnDevice(b.orbit) == 0
    out = _render(r, b, T, n)
    assert np.array_equal(out, ref_b) and np.array_equal(out, _fresh_frame(native_libs, b, n, built=True))
    assert r.read_bla_native()["heap_records"].tobytes() == b.derived.heap_records.tobytes()
    # the table uploaded first and the orbit after it
    _install(r, a, built=False)
    assert r._lib.fs_upload_bla(r._h, T, b.bla.level_ptrs, b.bla.level_sizes, b.bla.num_levels, b.bla.lm2) == 0
    _upload_orbit(r, b)
    out = _render(r, b, T, n)
    assert np.array_equal(out, ref_b) and np.array_equal(out, _fresh_frame(native_libs, b, n, built=False))
    assert r.read_bla_native()["heap_records"].tobytes() == b.derived.heap_records.tobytes()
    # an HDRFloat<double> table after a float one, and a float one after that
    d = bm.case(19, 257, True)
    T64 = _install(r, d, built=True)
    ref_d = _oracle.bla_hdr32(d.view, d.orbit, d.bla, n_iterations=n)
    assert np.array_equal(_render(r, d, T64, n), ref_d)
    with pytest.raises(RuntimeError):  # (no native form of a double table: FS_ERR_6)
        r.read_bla_native()
    T = _install(r, b, built=True)
    out = _render(r, b, T, n)
    assert np.array_equal(out, ref_b)
    g = r.read_bla_native()
    assert g["heap_ok"] and g["heap_records"].tobytes() == b.derived.heap_records.tobytes()
    assert g["q"].tobytes() == b.derived.q.tobytes()
