"""The form without the dz add (NDZ) of the hand-scheduled body of k_lav2_hdr32_fast (FS_FAST_LOOP_FDU in csrc/scaled_runs.hpp).

Where |dz| is far enough below |Z| the first instruction of a scaled step, s = fma(w, 2^E, 2Z), returns 2Z bit for bit; an NDZ body
multiplies by the entry's 2Z directly, three packed instructions a step.  Whether the next eight steps may do that is decided where a
body ends, from the orbit alone: max|w| against T2 = min(NDZ body bound - largest scale shift, bits(2^-5)), the bound being the third
companion array k_make_quiet_orbit writes.  NDZ bodies are reachable from the add-free (ND) loop only.  What is held here:

  1. the tuned kernel's frame is the literal transcription's, pixel for pixel -- View 5 (where NDZ carries steps; both stage-test
     directions, Full and perturbation only), View 3 and the generated shallow views (where it carries few or none), the deep views
     11, 14 and 19 (scale shifts far below -2^30: the "never" and overflow corners of T2 are live), and an orbit whose last entries
     are crafted so that bodies end on entries whose bound must be "never" -- and the CPU oracle's on View 5 and the shallow views;
  2. REPLAY: the counting instantiation runs every accepted add-free invocation again in the full form, NDZ bodies included, and
     compares end state bits, max|w|, step count, status and the hand-over values: no mismatch, anywhere;
  3. the form is really used: on View 5 at 64x36 NDZ carries at least a quarter of the add-free wave-steps;
  4. fallback: at a width of 1e-6 no add-free run starts, so no NDZ step is taken; the full form carries steps on every shallow view;
  5. T2 itself, evaluated on the device by the macro the loop uses (FS_BT_T2), against its definition at the corners.

Statistics words (fs_read_stats_raw): 8 = four-step blocks taken inside the statement (any form), 30 = add-free wave-steps (NDZ
included), 31 = unused, 32 = failed ND verdicts, 33 = replay mismatches, 34 = invocations replayed, 35 = NDZ wave-steps."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle
import _truth
from fractalshark_amd import GPURenderer, LAV2_FULL, LAV2_PO, PARITY_CPU, PARITY_CPU_GPUSTAGE, T_HDR32, inputs

pytestmark = pytest.mark.gpu

W_BLOCKS, W_ND, W_UNUSED, W_FAIL, W_MISMATCH, W_REPLAYED, W_NDZ = 8, 30, 31, 32, 33, 34, 35
SHALLOW = ["shallow_1e-6", "shallow_1e-12", "shallow_1e-28"]
DEEP_CAP = 100000  # iteration cap of the deep views: the perturbation loop still runs tens of thousands of steps per pixel
HZ = 0x3D000000    # bits(2^-5)
NEVER = -(1 << 31)


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.enable_step_count(False)
    r.set_kernel_variant(0)
    r.close()


def _crafted_orbit(v, mild):
    """View 5's orbit with scaled entries near its end: bodies whose eight entries would cross them, or the orbit's end, must find
    the "never" bound.  Not mild: period-boundary-like entries (tiny |Z|) among the last sixteen and a few further in (the LA table
    built from them takes most steps); mild: the last twelve entries a quarter of their size (the table stays as it was)."""
    ob = inputs.Orbit(v)
    last = ob.count - 1
    if mild:
        idx = [last - k for k in range(1, 13)]
        ex = [-2] * len(idx)
    else:
        idx = [last - 1, last - 4, last - 9, last - 15, last // 2, last // 2 + 1, last // 3]
        ex = [-30, -50, -20, -40, -30, -50, -24]
    assert ob.scale_entries(idx, ex) == len(idx)
    return ob


@functools.lru_cache(maxsize=None)
def _inputs(name):
    if name.startswith("view"):
        n, size = name.split("_")[:2]
        w, h = (int(x) for x in size.split("x"))
        v = inputs.View.builtin(int(n[4:]), w, h)
    else:
        v = _truth.Case(name).view(inputs)
    ob = _crafted_orbit(v, name.endswith("_mild")) if "_crafted" in name else inputs.Orbit(v)
    return v, ob, inputs.LATable(ob)


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, mode, stage_test):
    v, ob, la = _inputs(name)
    out = _oracle.lav2_hdr32(v, ob, la, stage_test=stage_test) if mode == LAV2_FULL else _oracle.bla_hdr32(v, ob, None)
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


def _st(parity):
    return 0 if parity == PARITY_CPU else 1


def _check_counts(name, raw):
    print("ndz %-20s statement wave-steps %d  add-free %d  NDZ %d  failed verdicts %d  replayed %d  mismatches %d"
          % (name, 4 * raw[W_BLOCKS], raw[W_ND], raw[W_NDZ], raw[W_FAIL], raw[W_REPLAYED], raw[W_MISMATCH]))
    assert raw[W_MISMATCH] == 0, (name, raw[W_MISMATCH])
    assert raw[W_UNUSED] == 0
    assert raw[W_NDZ] <= raw[W_ND] <= 4 * raw[W_BLOCKS], (name, raw[W_NDZ], raw[W_ND], 4 * raw[W_BLOCKS])
    assert raw[W_ND] == 0 or raw[W_REPLAYED] > 0


# ---- 1. bit-equality where NDZ carries steps, 2. replay
@pytest.mark.parametrize("parity", [PARITY_CPU, PARITY_CPU_GPUSTAGE])
@pytest.mark.parametrize("name", ["view5_64x36", "view5_256x144"])
def test_view5_full_equals_the_literal_variant_and_the_oracle(renderer, native_libs, name, parity):
    tuned, _ = _render(renderer, name, LAV2_FULL, parity)
    lit, _ = _render(renderer, name, LAV2_FULL, parity, literal=True)
    assert np.array_equal(tuned, lit), (name, parity, int((tuned != lit).sum()))
    if name == "view5_64x36":
        ref = _oracle_frame(name, LAV2_FULL, _st(parity))
        assert np.array_equal(tuned, ref), (name, parity, int((tuned != ref).sum()))
    counted, raw = _counting(renderer, name, LAV2_FULL, parity)
    assert np.array_equal(counted, tuned), (name, parity)
    _check_counts(name, raw)
    assert raw[W_REPLAYED] > 0, raw[W_REPLAYED]
    if parity == PARITY_CPU:
        # (with the LA stages in use the perturbation loop starts where dz is no longer 2^26 below Z: the statement sees 8 924
        # wave-steps at 64x36, all of them add-free, none of them NDZ -- measured, and no defect)
        assert raw[W_NDZ] > 0, raw[W_NDZ]


def test_view5_perturbation_only_equals_the_literal_variant(renderer, native_libs):
    name = "view5_64x36"
    tuned, _ = _render(renderer, name, LAV2_PO, PARITY_CPU)
    lit, _ = _render(renderer, name, LAV2_PO, PARITY_CPU, literal=True)
    assert np.array_equal(tuned, lit), int((tuned != lit).sum())
    counted, raw = _counting(renderer, name, LAV2_PO, PARITY_CPU)
    assert np.array_equal(counted, tuned)
    _check_counts(name + " po", raw)  # (perturbation only asks for no add-free run, before this form and with it)


# ---- 4. fallback
@pytest.mark.parametrize("name", SHALLOW + ["view3_64x36"])
def test_shallow_views_and_view3(renderer, native_libs, name):
    tuned, _ = _render(renderer, name, LAV2_FULL, PARITY_CPU)
    lit, _ = _render(renderer, name, LAV2_FULL, PARITY_CPU, literal=True)
    assert np.array_equal(tuned, lit), (name, int((tuned != lit).sum()))
    if name in SHALLOW:
        ref = _oracle_frame(name, LAV2_FULL, 0)
        assert np.array_equal(tuned, ref), (name, int((tuned != ref).sum()))
    counted, raw = _counting(renderer, name, LAV2_FULL, PARITY_CPU)
    assert np.array_equal(counted, tuned), name
    _check_counts(name, raw)
    if name in SHALLOW:
        assert 4 * raw[W_BLOCKS] - raw[W_ND] > 0, (name, raw[W_BLOCKS], raw[W_ND])  # the full form carries steps
    if name == "shallow_1e-6":
        # no add-free entry vote can pass there (tests/test_gpu_lav2_add_free.py gives the reason), and NDZ is entered from ND only
        assert raw[W_NDZ] == 0 and raw[W_ND] == 0, (raw[W_NDZ], raw[W_ND])


# ---- the deep views: scale shifts far below -2^30
@pytest.mark.parametrize("view", [11, 14, 19])
def test_deep_views_equal_the_literal_variant(renderer, native_libs, view):
    name = "view%d_64x36" % view
    tuned, _ = _render(renderer, name, LAV2_FULL, PARITY_CPU, cap=DEEP_CAP)
    lit, _ = _render(renderer, name, LAV2_FULL, PARITY_CPU, literal=True, cap=DEEP_CAP)
    assert np.array_equal(tuned, lit), (name, int((tuned != lit).sum()))
    counted, raw = _counting(renderer, name, LAV2_FULL, PARITY_CPU, cap=DEEP_CAP)
    assert np.array_equal(counted, tuned), name
    _check_counts(name, raw)


# ---- bodies that would read bounds across the orbit's end, or across an entry nothing may arrive at
@pytest.mark.parametrize("name,mode", [("view5_64x36_crafted", LAV2_FULL), ("view5_64x36_crafted", LAV2_PO),
                                       ("view5_64x36_crafted_mild", LAV2_FULL)])
def test_crafted_orbit_with_boundaries_near_its_end(renderer, native_libs, name, mode):
    tuned, _ = _render(renderer, name, mode, PARITY_CPU, cap=DEEP_CAP)
    lit, _ = _render(renderer, name, mode, PARITY_CPU, literal=True, cap=DEEP_CAP)
    assert np.array_equal(tuned, lit), (mode, int((tuned != lit).sum()))
    counted, raw = _counting(renderer, name, mode, PARITY_CPU, cap=DEEP_CAP)
    assert np.array_equal(counted, tuned)
    _check_counts(name, raw)


# ---- 3. not vacuous
def test_ndz_carries_a_quarter_of_the_add_free_steps_of_view5(renderer, native_libs):
    _, raw = _counting(renderer, "view5_64x36", LAV2_FULL, PARITY_CPU)
    nd, ndz = raw[W_ND], raw[W_NDZ]
    print("View 5 64x36: statement wave-steps %d, add-free %d, NDZ %d (%.1f %% of the add-free steps)"
          % (4 * raw[W_BLOCKS], nd, ndz, 100.0 * ndz / max(1, nd)))
    assert nd > 0 and raw[W_REPLAYED] > 0
    assert 4 * ndz >= nd, (ndz, nd)


# ---- 5. the threshold
def _model(bound, shift, dc):
    if dc > bound:
        return -1
    return min(bound - shift, HZ)


def test_ndz_threshold_corners_and_random(native_libs):
    rng = np.random.default_rng(8)
    shifts = [-254 << 23, -200 << 23, -129 << 23, -(1 << 30) - 1, -(1 << 30), -128 << 23, -127 << 23, -1 << 23, 0, 1 << 23,
              64 << 23, 127 << 23]
    bounds = [NEVER, 0, 1, 0x00800000, 0x03800000, 0x33800000, 0x3C800000, HZ - 1, HZ, HZ + 1, 0x3F800000, 0x46800000, 0x7F000000,
              0x7F7FFFFF]
    dcs = [0, 1, 0x00800000, 0x33800000, HZ, 0x3F800000, 0x7F000000, 0x7F800000]
    cases = [(b, s, d) for b in bounds for s in shifts for d in dcs]
    # max|dc| just below, at and just above the bound
    cases += [(b, s, b + k) for b in bounds[1:-1] for s in (-200 << 23, 0) for k in (-1, 0, 1) if b + k >= 0]
    for _ in range(4000):
        b = NEVER if rng.random() < 0.1 else int(rng.integers(0, 0x7F800000))
        s = int(rng.integers(-254, 128)) << 23
        d = int(rng.integers(0, 0x7F800001))
        cases.append((b, s, d))
    bw = np.array([c[0] for c in cases], dtype=np.int32)
    sh = np.array([c[1] for c in cases], dtype=np.int32)
    dc = np.array([c[2] for c in cases], dtype=np.int32)
    out = np.zeros(len(cases), dtype=np.int32)
    r = GPURenderer(0)
    try:
        rc = r._lib.fs_test_ndz_threshold(r._h, bw.ctypes.data_as(C.c_void_p), sh.ctypes.data_as(C.c_void_p),
                                          dc.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(cases))
    finally:
        r.close()
    assert rc == 0
    want = np.array([_model(*c) for c in cases], dtype=np.int64)
    bad = np.nonzero(out.astype(np.int64) != want)[0]
    assert bad.size == 0, [(cases[i], int(out[i]), int(want[i])) for i in bad[:8]]
    assert (out[bw == NEVER] < 0).all()   # a "never" bound yields a threshold no bit pattern of max|w| (>= 0) can pass
    assert (out <= HZ).all()              # clamped at Hz
