"""The add-free (ND, "no dc") form of the hand-scheduled body of k_lav2_hdr32_fast (FS_FAST_LOOP_FDU in csrc/scaled_runs.hpp).

On a deep view the last instruction of a scaled step, q = p + dc 2^-E, returns p bit for bit; the ND form leaves it out, certifies
that with one per-lane compare when the statement ends (the smallest part of every state against F_run = max(2^-56, 2^26 max|dcs|))
and repeats the run in the full form when the compare fails.  What is held here:

  1. the tuned kernel's frame is the literal transcription's, pixel for pixel, and the CPU oracle's (View 5, where ND carries the
     statement's steps; both stage-test directions; Full and perturbation only);
  2. the same on shallower views (the generated shallow views, View 3): where dc is not negligible the entry vote or the verdict
     sends the runs to the full form, which carries steps on every one of them -- all of them at a width of 1e-6 and 1e-12; at
     1e-28 and on View 3 dz soon grows 2^26 above dc and both forms carry steps;
  3. REPLAY: the counting instantiation runs every accepted ND invocation of the statement again, from the same start, in the full
     form and compares end state bits, step count, status and what the statement hands to the tested block: no mismatch, anywhere;
  4. the form is really used: on View 5 at 64x36 ND carries at least half of the statement's wave-steps (the CPU model of the
     condition gives 100 % of them there).

Statistics words (fs_read_stats_raw): 8 = four-step blocks taken inside the statement (either form), 30 = wave-steps in ND,
32 = failed ND verdicts, 33 = replay mismatches, 34 = invocations replayed.  (Word 31 is kept for a form without the dz add, which
this kernel does not have: DESIGN.md section 7.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle
import _truth
from fractalshark_amd import GPURenderer, LAV2_FULL, LAV2_PO, PARITY_CPU, PARITY_CPU_GPUSTAGE, T_HDR32, inputs

pytestmark = pytest.mark.gpu

W_BLOCKS, W_ND, W_NDZ, W_FAIL, W_MISMATCH, W_REPLAYED = 8, 30, 31, 32, 33, 34
SHALLOW = ["shallow_1e-6", "shallow_1e-12", "shallow_1e-28"]
# (case, mode, parity): the inputs of the tests 1 and 2 -- each rendered once by the counting instantiation, for 2, 3 and 4
COUNTED = [("view5_64x36", LAV2_FULL, PARITY_CPU), ("view5_64x36", LAV2_FULL, PARITY_CPU_GPUSTAGE), ("view5_64x36", LAV2_PO, PARITY_CPU),
           ("view5_256x144", LAV2_FULL, PARITY_CPU), ("view5_256x144", LAV2_FULL, PARITY_CPU_GPUSTAGE)] + \
          [(n, LAV2_FULL, PARITY_CPU) for n in SHALLOW + ["view3_64x36"]]


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.enable_step_count(False)
    r.set_kernel_variant(0)
    r.close()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    if name.startswith("view5_") or name.startswith("view3_"):
        n, size = name.split("_")
        w, h = (int(x) for x in size.split("x"))
        v = inputs.View.builtin(int(n[4:]), w, h)
    else:
        v = _truth.Case(name).view(inputs)
    ob = inputs.Orbit(v)
    return v, ob, inputs.LATable(ob)


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, mode, stage_test):
    v, ob, la = _inputs(name)
    # (perturbation only: the CPU twin is the perturbation function without a table, as in tests/test_gpu_parity.py)
    out = _oracle.lav2_hdr32(v, ob, la, stage_test=stage_test) if mode == LAV2_FULL else _oracle.bla_hdr32(v, ob, None)
    out.setflags(write=False)
    return out


def _render(r, name, mode, parity, literal=False, counting=False):
    v, ob, la = _inputs(name)
    assert r.set_kernel_variant(literal=literal) == 0
    r.enable_step_count(counting)
    try:
        assert r.InitializeMemory(v.width, v.height, 1, None, 0, 0, 0, False) == 0
        assert r.InitializePerturb(1, ob, 0, None, la) == 0
        assert r.ClearMemory() == 0
        co = [(float(c["m"]), int(c["e"])) for c in v.coords_perturb(ob)]
        assert r.RenderPerturbLAv2(None, None, None, *co, v.num_iterations, T=T_HDR32, Mode=mode, parity=parity) == 0
        assert r.SyncComputeStream() == 0
        raw = None
        if counting:
            buf = (C.c_uint64 * 40)()
            assert r._lib.fs_read_stats_raw(r._h, buf, 40) == 0
            raw = [int(x) for x in buf]
        out = r.new_iter_buffer()
        assert r.RenderCurrent(v.num_iterations, out) == 0
        assert r.SyncComputeStream() == 0
        return out, raw
    finally:
        r.enable_step_count(False)
        r.set_kernel_variant(literal=False)


_counted = {}


def _counting(r, name, mode, parity):
    key = (name, mode, parity)
    if key not in _counted:
        _counted[key] = _render(r, name, mode, parity, counting=True)
    return _counted[key]


def _st(parity):
    return 0 if parity == PARITY_CPU else 1


# ---- 1. bit-equality where the add-free form carries the steps
@pytest.mark.parametrize("parity", [PARITY_CPU, PARITY_CPU_GPUSTAGE])
@pytest.mark.parametrize("name", ["view5_64x36", "view5_256x144"])
def test_view5_full_equals_the_literal_variant_and_the_oracle(renderer, native_libs, name, parity):
    tuned, _ = _render(renderer, name, LAV2_FULL, parity)
    lit, _ = _render(renderer, name, LAV2_FULL, parity, literal=True)
    assert np.array_equal(tuned, lit), (name, parity, int((tuned != lit).sum()))
    if name == "view5_64x36":
        ref = _oracle_frame(name, LAV2_FULL, _st(parity))
        assert np.array_equal(tuned, ref), (name, parity, int((tuned != ref).sum()))


def test_view5_perturbation_only_equals_the_literal_variant_and_the_oracle(renderer, native_libs):
    name = "view5_64x36"
    tuned, _ = _render(renderer, name, LAV2_PO, PARITY_CPU)
    lit, _ = _render(renderer, name, LAV2_PO, PARITY_CPU, literal=True)
    ref = _oracle_frame(name, LAV2_PO, 0)
    assert np.array_equal(tuned, lit), int((tuned != lit).sum())
    assert np.array_equal(tuned, ref), int((tuned != ref).sum())


# ---- 2. fallback: dc is not negligible, the full form carries steps, the frame is still the literal variant's and the oracle's
@pytest.mark.parametrize("name", SHALLOW + ["view3_64x36"])
def test_fallback_where_dc_is_not_negligible(renderer, native_libs, name):
    tuned, _ = _render(renderer, name, LAV2_FULL, PARITY_CPU)
    lit, _ = _render(renderer, name, LAV2_FULL, PARITY_CPU, literal=True)
    ref = _oracle_frame(name, LAV2_FULL, 0)
    assert np.array_equal(tuned, lit), (name, int((tuned != lit).sum()))
    assert np.array_equal(tuned, ref), (name, int((tuned != ref).sum()))
    counted, raw = _counting(renderer, name, LAV2_FULL, PARITY_CPU)
    assert np.array_equal(counted, tuned), name
    statement, nd = 4 * raw[W_BLOCKS], raw[W_ND]
    print("add-free %-14s statement wave-steps %d  ND %d  failed verdicts %d  replayed %d" % (name, statement, nd, raw[W_FAIL], raw[W_REPLAYED]))
    assert raw[W_NDZ] == 0
    assert statement - nd > 0, (name, statement, nd)  # the full form carries steps
    if name == "shallow_1e-6":
        # a priori: the pixel spacing is 1e-6 / 64 > 2^-26, so some lane of every 8x8 tile has max|dc| > 2^-26 and its F_run is
        # above 1 in true scale, while a scaled step keeps |dz| below 0.354 |Z| < 1: no entry vote can pass
        assert nd == 0 and raw[W_FAIL] == 0, (nd, raw[W_FAIL])


# ---- 3. replay
@pytest.mark.parametrize("name,mode,parity", COUNTED)
def test_replay_in_the_full_form_ends_where_the_add_free_form_ended(renderer, native_libs, name, mode, parity):
    counted, raw = _counting(renderer, name, mode, parity)
    tuned, _ = _render(renderer, name, mode, parity)
    assert np.array_equal(counted, tuned), (name, mode, parity)  # the counting instantiation renders the product's frame
    print("replay %-14s mode %d parity %d: ND wave-steps %d, replayed %d, mismatches %d, failed verdicts %d"
          % (name, mode, parity, raw[W_ND], raw[W_REPLAYED], raw[W_MISMATCH], raw[W_FAIL]))
    assert raw[W_MISMATCH] == 0, raw[W_MISMATCH]
    assert raw[W_ND] == 0 or raw[W_REPLAYED] > 0  # add-free steps were taken: their invocations have been replayed


# ---- 4. not vacuous
def test_the_add_free_form_carries_view5(renderer, native_libs):
    _, raw = _counting(renderer, "view5_64x36", LAV2_FULL, PARITY_CPU)
    statement, nd = 4 * raw[W_BLOCKS], raw[W_ND]
    print("View 5 64x36: statement wave-steps %d, ND %d (%.1f %%), failed verdicts %d" % (statement, nd, 100.0 * nd / max(1, statement), raw[W_FAIL]))
    assert statement > 0
    assert 2 * (nd + raw[W_NDZ]) >= statement, (nd, statement)
    assert raw[W_REPLAYED] > 0
