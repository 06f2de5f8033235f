"""The NDZ body bounds with the growth an NDZ body really has (ndz_body_bound in csrc/kernels_orbit_prep.hip; the argument is written out there and
under "NDZ" in csrc/scaled_runs.hpp).

An NDZ body of FS_FAST_LOOP_FDU multiplies dz by the entry's 2Z without adding dz to it first.  With D = max|dz| and C = max|dc| where the
body starts, lo = the smaller |part| of a 2Z, s_k = (|2Z_k.re| + |2Z_k.im|)(1 + 2^-10), A_m the product of the s of the steps before m
and B_m = s B_(m-1) + 1, entry j has two bounds: D <= the smallest 2^-27 lo_(j+m) / A_m, m = 0 .. 7, and C <= the smallest
2^-27 lo_(j+m) / B_m, m = 1 .. 7, each also within half of scaled_bound(Z_(j+8)) over A_8 / B_8, times (1 - 2^-10).  The parent commit had
ONE bound on max(D, C) and divided by the block bound's growth (4 M + 3.8 a step), some 2^10 more over a body.  What is held here:

  1. the tuned kernel's frame is the literal transcription's and the CPU oracle's, pixel for pixel, on every case (the oracle's
     frame is rendered once per case; View 5 at 256x144 with parity cpu and View 14 cost it a quarter of a minute each): View 5 in
     both stage-test directions and perturbation only, View 3, the generated shallow views, the deep views 11, 14 and 19, the two
     crafted orbits of tests/test_gpu_lav2_ndz.py and a third one, View 5's orbit with sixteen consecutive near-axis entries in its
     middle (one part of 2Z 2^-30 of the other: lo collapses there and |2Z.re| + |2Z.im| does not, which is where the new growth
     and the old one differ most);
  2. REPLAY: the counting instantiation runs every accepted add-free invocation again in the full form -- statistics word 33
     (mismatches) is 0 and word 34 (invocations replayed) is not, for every case of 1. that has an add-free invocation at all (two
     cannot: perturbation only, and the width of 1e-6; they are held to have none): s == 2Z held wherever the bound said so;
  3. the bounds against their definition by brute force: read back (fs_read_ndz_bounds), every entry with bounds is started from worst-case
     and seeded random states within them (dz within the first, dc within the second) and stepped eight times in binary32, each operation rounded once as the full form rounds it:
     fl(fma(w, 2^E, 2Z)) == 2Z in both parts at every step, every arrival within its entry's own bound; entries whose window holds an
     unusable entry or crosses the orbit's end read "never";
  4. not vacuous: on View 5 at 64x36 NDZ carries more than the parent's 270 520 of 838 004 statement wave-steps, and the add-free forms
     together not fewer than its 688 972 (profiles/r08_ndz_ab.json).

Statistics words (fs_read_stats_raw): 8 = four-step blocks taken inside the statement, 30 = add-free wave-steps (NDZ included), 32 = failed
ND verdicts, 33 = replay mismatches, 34 = invocations replayed, 35 = NDZ wave-steps."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle
import test_gpu_lav2_ndz as base
from _quiet_model import start_states as _start_states  # (shared with tests/test_quiet_model_cpu.py)
from fractalshark_amd import GPURenderer, LAV2_FULL, LAV2_PO, PARITY_CPU, PARITY_CPU_GPUSTAGE, T_HDR32, inputs

pytestmark = pytest.mark.gpu

W_BLOCKS, W_ND, W_FAIL, W_MISMATCH, W_REPLAYED, W_NDZ = 8, 30, 32, 33, 34, 35
NEVER_BITS = 0x80000000
PARENT_STATEMENT, PARENT_ND, PARENT_NDZ = 838004, 688972, 270520  # View 5, 64x36, parity cpu: profiles/r08_ndz_ab.json
NEAR_AXIS = "view5_64x36_nearaxis"
CRAFTED = ["view5_64x36_crafted", "view5_64x36_crafted_mild", NEAR_AXIS]


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.enable_step_count(False)
    r.set_kernel_variant(0)
    r.close()


def _near_axis_orbit(v):
    """View 5's orbit with sixteen consecutive entries in its middle turned towards an axis: the smaller part of each becomes 2^-30 of
    the larger one (alternately the real and the imaginary axis would need the larger part moved; the larger part stays as it is)."""
    ob = inputs.Orbit(v)
    e = ob.entries()
    idx = np.arange(ob.count // 2, ob.count // 2 + 16)
    re_larger = e["ex"][idx] >= e["ey"][idx]
    d_re = np.where(re_larger, 0, e["ey"][idx] - 30 - e["ex"][idx])
    d_im = np.where(re_larger, e["ex"][idx] - 30 - e["ey"][idx], 0)
    assert ob.scale_parts(idx, d_re, d_im) == idx.size
    e = ob.entries()
    assert (np.abs(e["ex"][idx] - e["ey"][idx]) == 30).all()
    return ob


@functools.lru_cache(maxsize=None)
def _inputs(name):
    if name != NEAR_AXIS:
        return base._inputs(name)
    v = inputs.View.builtin(5, 64, 36)
    ob = _near_axis_orbit(v)
    return v, ob, inputs.LATable(ob)


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, mode, stage_test, cap):
    v, ob, la = _inputs(name)
    n = v.num_iterations if cap is None else min(v.num_iterations, cap)
    if mode == LAV2_FULL:
        out = _oracle.lav2_hdr32(v, ob, la, stage_test=stage_test, n_iterations=n)
    else:
        out = _oracle.bla_hdr32(v, ob, None, n_iterations=n)
    out.setflags(write=False)
    return out


def _render(r, name, mode, parity, literal=False, counting=False, cap=None):
    v, ob, la = _inputs(name)
    n = v.num_iterations if cap is None else min(v.num_iterations, cap)
    assert r.set_kernel_variant(literal=literal) == 0
    r.enable_step_count(counting)
    try:
        assert r.InitializeMemory(v.width, v.height, 1, None, 0, 0, 0, False) == 0
        assert r.InitializePerturb(1, ob, 0, None, la) == 0
        assert r.ClearMemory() == 0
        co = [(float(c["m"]), int(c["e"])) for c in v.coords_perturb(ob)]
        assert r.RenderPerturbLAv2(None, None, None, *co, n, T=T_HDR32, Mode=mode, parity=parity) == 0
        assert r.SyncComputeStream() == 0
        raw = None
        if counting:
            buf = (C.c_uint64 * 40)()
            assert r._lib.fs_read_stats_raw(r._h, buf, 40) == 0
            raw = [int(x) for x in buf]
        out = r.new_iter_buffer()
        assert r.RenderCurrent(n, out) == 0
        assert r.SyncComputeStream() == 0
        return out, raw
    finally:
        r.enable_step_count(False)
        r.set_kernel_variant(literal=False)


_counted = {}


def _counting(r, name, mode, parity, cap=None):
    key = (name, mode, parity, cap)
    if key not in _counted:
        _counted[key] = _render(r, name, mode, parity, counting=True, cap=cap)
    return _counted[key]


# ---- 1. frame equality, 2. replay
CASES = (
    [("view5_64x36", LAV2_FULL, p, None, True) for p in (PARITY_CPU, PARITY_CPU_GPUSTAGE)] +
    [("view5_256x144", LAV2_FULL, p, None, True) for p in (PARITY_CPU, PARITY_CPU_GPUSTAGE)] +
    [("view5_64x36", LAV2_PO, PARITY_CPU, None, True), ("view3_64x36", LAV2_FULL, PARITY_CPU, None, True)] +
    [(n, LAV2_FULL, PARITY_CPU, None, True) for n in base.SHALLOW] +
    [("view%d_64x36" % n, LAV2_FULL, PARITY_CPU, base.DEEP_CAP, True) for n in (11, 14, 19)] +
    [(n, LAV2_FULL, PARITY_CPU, base.DEEP_CAP, True) for n in CRAFTED[:2]] +
    # (under the cap the pixels of this orbit stop before dz has grown 2^26 above dc: no add-free step; without it 218 196)
    [(NEAR_AXIS, LAV2_FULL, PARITY_CPU, None, True)])
# Cases that cannot be replayed because no add-free invocation exists: perturbation only asks for no add-free run, and at a width
# of 1e-6 no entry vote can pass (tests/test_gpu_lav2_add_free.py gives the reason; tests/test_gpu_lav2_nd_backoff.py holds it).
NOTHING_TO_REPLAY = {("view5_64x36", LAV2_PO), ("shallow_1e-6", LAV2_FULL)}


@pytest.mark.parametrize("name,mode,parity,cap,oracle", CASES,
                         ids=["%s-%s-%s" % (c[0], "full" if c[1] == LAV2_FULL else "po", "cpu" if c[2] == PARITY_CPU else "gpustage")
                              for c in CASES])
def test_frame_equals_literal_variant_and_oracle_and_replay_agrees(renderer, native_libs, name, mode, parity, cap, oracle):
    tuned, _ = _render(renderer, name, mode, parity, cap=cap)
    lit, _ = _render(renderer, name, mode, parity, literal=True, cap=cap)
    assert np.array_equal(tuned, lit), (name, mode, parity, int((tuned != lit).sum()))
    if oracle:
        ref = _oracle_frame(name, mode, base._st(parity), cap)
        assert np.array_equal(tuned, ref), (name, mode, parity, int((tuned != ref).sum()))
    counted, raw = _counting(renderer, name, mode, parity, cap=cap)
    assert np.array_equal(counted, tuned), (name, mode, parity)
    print("ndz-tight %-26s statement wave-steps %d  add-free %d  NDZ %d  failed verdicts %d  replayed %d  mismatches %d"
          % (name, 4 * raw[W_BLOCKS], raw[W_ND], raw[W_NDZ], raw[W_FAIL], raw[W_REPLAYED], raw[W_MISMATCH]))
    assert raw[W_MISMATCH] == 0, (name, raw[W_MISMATCH])
    if (name, mode) in NOTHING_TO_REPLAY:
        assert raw[W_ND] == 0 and raw[W_REPLAYED] == 0, (name, raw[W_ND], raw[W_REPLAYED])
    else:
        assert raw[W_REPLAYED] > 0, (name, raw[W_REPLAYED])
    assert raw[W_NDZ] <= raw[W_ND] <= 4 * raw[W_BLOCKS], (name, raw[W_NDZ], raw[W_ND], 4 * raw[W_BLOCKS])


# ---- 3. the bound against its definition
def _read_bounds(r, name):
    """(bounds, entries): znz ({on max|dz|, on max|dc|} per entry) and the second companion {2Z.re, 2Z.im, own bound, block bound} of the orbit of `name`, its two spare
    entries dropped."""
    v, ob, la = _inputs(name)
    assert r.InitializeMemory(v.width, v.height, 1, None, 0, 0, 0, False) == 0
    assert r.InitializePerturb(1, ob, 0, None, la) == 0
    n = C.c_uint64(0)
    assert r._lib.fs_read_ndz_bounds(r._h, None, None, 0, C.byref(n)) == 0
    assert n.value == ob.count + 2, (n.value, ob.count)
    b = np.zeros((n.value, 2), np.float32)
    e = np.zeros((n.value, 4), np.float32)
    assert r._lib.fs_read_ndz_bounds(r._h, b.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), n.value, None) == 0
    return b[:ob.count], e[:ob.count]


@pytest.mark.parametrize("name", ["view5_64x36"] + CRAFTED)
def test_bound_against_its_definition(renderer, native_libs, name):
    bounds, ent = _read_bounds(renderer, name)
    n = bounds.shape[0]
    bits = np.ascontiguousarray(bounds[:, 0]).view(np.uint32)
    # (both bounds are "never" together)
    assert ((np.ascontiguousarray(bounds[:, 1]).view(np.uint32) == NEVER_BITS) == (bits == NEVER_BITS)).all()
    own_never = ent[:, 2].view(np.uint32) == NEVER_BITS
    has = bits != NEVER_BITS
    # "never" where the window j + 1 .. j + 8 holds an entry nothing may arrive at, or crosses the orbit's end
    # (the read-back counts the orbit's two spare entries; the orbit proper ends at n)
    bad_window = np.zeros(n, bool)
    for m in range(1, 9):
        bad_window[:n - m] |= own_never[m:]
        bad_window[n - m:] = True
    assert not (has & bad_window).any(), np.nonzero(has & bad_window)[0][:8]
    assert (bounds[has] >= 2.0 ** -120).all() and np.isfinite(bounds[has]).all()  # (both columns)
    j = np.nonzero(has)[0]
    print("ndz-tight %-26s entries %d, with a bound %d (%.1f %%)" % (name, n, j.size, 100.0 * j.size / n))
    assert j.size > 0
    st = _start_states(np.random.default_rng(9))
    b = bounds[j, 0].astype(np.float64)[:, None]
    bc = bounds[j, 1].astype(np.float64)[:, None]
    # the run's scale: w = dz 2^-E with max|w| near 2^-24, as a run starts (E a power of two: scaling changes no bit)
    E = np.floor(np.log2(b)) + 24.0
    sc, isc = np.exp2(E), np.exp2(-E)
    w_re = (st[None, :, 0] * b * isc).astype(np.float32)
    w_im = (st[None, :, 1] * b * isc).astype(np.float32)
    dc_re = (st[None, :, 2] * bc * isc).astype(np.float32)
    dc_im = (st[None, :, 3] * bc * isc).astype(np.float32)
    assert (np.abs(dc_re.astype(np.float64)) * sc <= bc).all() and (np.abs(dc_im.astype(np.float64)) * sc <= bc).all()
    # (rounding a state to binary32 must not carry it over the bound)
    assert (np.abs(w_re.astype(np.float64)) * sc <= b).all() and (np.abs(w_im.astype(np.float64)) * sc <= b).all()
    for m in range(8):
        z_re, z_im = ent[j + m, 0][:, None], ent[j + m, 1][:, None]
        # s = fma(w, 2^E, 2Z): evaluated in binary64, rounded to binary32 once
        s_re = (w_re.astype(np.float64) * sc + z_re.astype(np.float64)).astype(np.float32)
        s_im = (w_im.astype(np.float64) * sc + z_im.astype(np.float64)).astype(np.float32)
        ok = (s_re == z_re) & (s_im == z_im)
        assert ok.all(), (name, m, [(int(j[a]), int(c)) for a, c in zip(*np.nonzero(~ok))][:6])
        # the full form's step, each operation rounded once: p = w s (two products and a sum per part), q = p + dc 2^-E
        p_re = (w_re * s_re) - (w_im * s_im)
        p_im = (w_re * s_im) + (w_im * s_re)
        w_re, w_im = p_re + dc_re, p_im + dc_im
        assert w_re.dtype == np.float32 and w_im.dtype == np.float32
        # the arrival's own bound test: max|dz| <= scaled_bound of entry j + m + 1, true scale
        mx = np.maximum(np.abs(w_re), np.abs(w_im)).astype(np.float64) * sc
        own = ent[j + m + 1, 2].astype(np.float64)[:, None]
        ok = mx <= own
        assert ok.all(), (name, m, [(int(j[a]), int(c)) for a, c in zip(*np.nonzero(~ok))][:6])


# ---- 4. not vacuous
def test_ndz_carries_more_than_the_parent_on_view5(renderer, native_libs):
    _, raw = _counting(renderer, "view5_64x36", LAV2_FULL, PARITY_CPU)
    statement, nd, ndz = 4 * raw[W_BLOCKS], raw[W_ND], raw[W_NDZ]
    print("View 5 64x36: statement wave-steps %d, add-free %d (%.1f %%; parent %.1f %%), NDZ %d (%.1f %%; parent %.1f %%)"
          % (statement, nd, 100.0 * nd / max(1, statement), 100.0 * PARENT_ND / PARENT_STATEMENT,
             ndz, 100.0 * ndz / max(1, statement), 100.0 * PARENT_NDZ / PARENT_STATEMENT))
    assert ndz > PARENT_NDZ, (ndz, PARENT_NDZ)
    assert nd >= PARENT_ND, (nd, PARENT_ND)
