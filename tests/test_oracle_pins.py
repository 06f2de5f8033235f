"""CPU-only: pin the oracle (and the host input builders it is fed by) against the reference's OWN golden
vectors -- the CRC-64s of the PNG files in FractalSharkTest/TestRenderGoldens.cpp:84-97 -- and against the
committed fixtures.  A matching CRC pins the whole chain view -> GMP orbit -> LA/BLA table -> CPU render ->
palette -> PNG bit-exactly."""
import json
import os

import numpy as np
import pytest

import _oracle
import golden_cases
from fractalshark_amd import inputs

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_small.npz"))
W = H = 256  # kGoldenWidth / kGoldenHeight

GOLDEN_CRC = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden_crc.json")))


def assert_golden(it, name, crc64, num_iterations, aa=1):
    """The oracle's buffer for the reference's golden case `name`: its CRC-32 and sum are those committed in
    tests/golden/golden_crc.json (written only after the oracle's PNG reproduced the reference's CRC-64 literal), and where the
    pin library was built (oracle/_ref/libpngpin.so) the PNG of that buffer has the literal CRC-64 itself."""
    g = GOLDEN_CRC[name]
    assert g["png_crc64"] == crc64 and g["antialiasing"] == aa
    assert list(it.shape) == g["iter_buffer_shape"]
    assert golden_cases.buffer_crc32(it) == g["iter_buffer_crc32"], name
    assert int(it.astype(np.uint64).sum()) == g["iter_sum"], name
    if _oracle.pin_lib() is not None:
        assert _oracle.png_crc64(it, W, H, aa, num_iterations) == crc64


@pytest.fixture(scope="module")
def view5(native_libs):
    v = inputs.View.builtin(5, W, H)
    ob = inputs.Orbit(v)
    return v, ob


@pytest.mark.parametrize("aa,expected", [(1, "1275500d639ad02e"), (4, "39671027bacf2567")])
def test_golden_view0_cpu64(native_libs, aa, expected):
    v = inputs.View.builtin(0, W, H, antialiasing=aa)
    it = _oracle.direct_f64(v, aa=aa)
    assert_golden(it, "view0-cpu64" if aa == 1 else "view0-cpu64-aa%d" % aa, expected, v.num_iterations, aa)


def test_golden_view5_cpu32_perturbed_blav2_hdr(view5):
    v, ob = view5
    la = inputs.LATable(ob)
    it = _oracle.lav2_hdr32(v, ob, la, stage_test=0)
    assert_golden(it, "view5-cpu-bla-v2", "1233a56b293e7b08", v.num_iterations)


def test_golden_view5_cpu32_perturbed_bla_hdr(view5):
    v, ob = view5
    bla = inputs.BLATable(ob)
    it = _oracle.bla_hdr32(v, ob, bla)
    assert_golden(it, "view5-cpu32-bla-hdr", "634d826801d54979", v.num_iterations)


def test_view5_inputs_match_fixture(native_libs):
    v = inputs.View.builtin(5, 64, 36)
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    assert [ob.count, ob.period] == list(GOLD["view5_orbit_count_period"])
    assert ob.entries()[:64].tobytes() == GOLD["view5_orbit_head"].tobytes()
    assert ob.entries()[-64:].tobytes() == GOLD["view5_orbit_tail"].tobytes()
    assert [la.count, la.stage_count, int(la.use_at)] == list(GOLD["view5_la_count_stages"])
    assert la.stages().tobytes() == GOLD["view5_la_stages"].tobytes()
    assert la.records()[:32].tobytes() == GOLD["view5_la_head"].tobytes()
    assert v.coords_perturb_hdr32(ob).tobytes() == GOLD["view5_coords_hdr32_64x36"].tobytes()
    # entry 0 is the explicit zero entry with exponent INT32_MIN >> 3
    e0 = ob.entries()[0]
    assert (e0["mx"], e0["ex"], e0["ey"], e0["my"]) == (0.0, -268435456, -268435456, 0.0)


def test_oracle_reproduces_fixtures(native_libs):
    v0 = inputs.View.builtin(0, 64, 48)
    assert np.array_equal(_oracle.direct_f64(v0), GOLD["view0_direct_f64_64x48"])
    v = inputs.View.builtin(5, 64, 36)
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    bla = inputs.BLATable(ob)
    assert np.array_equal(_oracle.lav2_hdr32(v, ob, la, stage_test=0), GOLD["view5_lav2_cpu_64x36"])
    assert np.array_equal(_oracle.lav2_hdr32(v, ob, la, stage_test=1), GOLD["view5_lav2_gpustage_64x36"])
    assert np.array_equal(_oracle.bla_hdr32(v, ob, None), GOLD["view5_po_64x36"])
    assert np.array_equal(_oracle.bla_hdr32(v, ob, bla), GOLD["view5_bla_64x36"])


def test_oracle_thread_count_independent(native_libs):
    """Row claiming must not change results (Fractal.cpp:2523-2543)."""
    v = inputs.View.builtin(5, 64, 36)
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    a = _oracle.lav2_hdr32(v, ob, la, threads=1, stage_test=1)
    b = _oracle.lav2_hdr32(v, ob, la, threads=5, stage_test=1)
    assert np.array_equal(a, b)


def test_la_table_threading_replay_equivalent(native_libs):
    """The reference builds stage 0 of the LA table on min(count/50000, cores) threads (LAReference.cpp:236-251);
    View 5's orbit (16046 entries) is below the threshold, so every host_threads value gives the same table."""
    v = inputs.View.builtin(5, 64, 36)
    ob = inputs.Orbit(v)
    assert ob.count < 50000
    a = inputs.LATable(ob, host_threads=1).records().tobytes()
    b = inputs.LATable(ob, host_threads=8).records().tobytes()
    assert a == b


# ---- HDRFloat<double> family and the HDR direct functions: five more of the reference's golden CRCs
def test_golden_view5_cpu64_perturbed_blav2_hdr(native_libs):
    v = inputs.View.builtin(5, W, H)
    ob = inputs.Orbit(v, is64=True)
    la = inputs.LATable(ob)
    it = _oracle.lav2_hdr32(v, ob, la, stage_test=0)
    assert_golden(it, "view5-cpu64-bla-v2", "ca7ad7c5f9cf750e", v.num_iterations)


def test_golden_view5_cpu64_perturbed_bla_hdr(native_libs):
    v = inputs.View.builtin(5, W, H)
    ob = inputs.Orbit(v, is64=True)
    bla = inputs.BLATable(ob)
    it = _oracle.bla_hdr32(v, ob, bla)
    assert_golden(it, "view5-cpu64-bla-hdr", "c91e33c3eb85b33d", v.num_iterations)


def test_golden_view1_cpu64_perturbed_bla_hdr(native_libs):
    v = inputs.View.builtin(1, W, H)
    ob = inputs.Orbit(v, is64=True)
    bla = inputs.BLATable(ob)
    it = _oracle.bla_hdr32(v, ob, bla)
    assert_golden(it, "view1-cpu-bla", "d0c8921c878f6dc3", v.num_iterations)


@pytest.mark.parametrize("is64,expected", [(False, "66ba2caaaa7f8013"), (True, "1275500d639ad02e")])
def test_golden_view0_cpuhdr(native_libs, is64, expected):
    v = inputs.View.builtin(0, W, H)
    it = _oracle.direct_hdr(v, is64)
    assert_golden(it, "view0-cpuhdr64" if is64 else "view0-cpuhdr", expected, v.num_iterations)


# ---- PerturbExtras::SimpleCompression ("RC" algorithms): compressed reference orbit + runtime decompression
@pytest.mark.parametrize("is64,expected", [(False, "b956600cfdfe431a"), (True, "68df9ceecaf1a667")])
def test_golden_view5_rc_blav2_hdr(native_libs, is64, expected):
    v = inputs.View.builtin(5, W, H)
    ob = inputs.Orbit(v, is64=is64, compression_exp=20)
    assert ob.compressed_count < ob.count
    la = inputs.LATable(ob)
    it = _oracle.lav2_hdr32(v, ob, la, stage_test=0)
    assert_golden(it, "view5-cpu64-rc-bla-v2" if is64 else "view5-cpu32-rc-bla-v2", expected, v.num_iterations)


def test_golden_view5_cpu64_perturbed_bla_plain_double(native_libs):
    """The twelfth golden: plain-double perturbation + BLA (Cpu64PerturbedBLA)."""
    v = inputs.View.builtin(5, W, H)
    ob = inputs.OrbitF64(v)
    it = _oracle.bla_f64(v, ob)
    assert_golden(it, "view5-cpu-perturbed-bla", "f201db00ade569fc", v.num_iterations)
