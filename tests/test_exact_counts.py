"""Every CPU oracle function against exact escape counts (tests/golden/exact_counts.json, tests/_truth.py).

The exact count of a sample is the first n with |z_n|^2 > R under z -> z^2 + c, iterated in GMP integers at the view's precision
(tests/truth/exact_counts.cpp): a reference that shares no text with oracle/ or the product.  On samples whose exact count does
not move when c moves by frame-width / 2^level, a path's output must EQUAL what its rule makes of the exact count (the rules and
the reference lines they come from: tests/_truth.py).  No shares, no iteration tolerances; capped samples are compared too.

  * The reference-pinned oracle paths (HDRFloat<float>, HDRFloat<double>, double; PO / BLA / LAv2 / direct) chose each case's
    level in the generator; here they must reproduce zero misses at it, on a stable set of at least 100 samples and 20 %.
  * The unpinned restatements (HDRFloat<CudaDblflt> LAv2, plain-type LAv2 in f32 / f64 / 2x32, the five low-precision direct
    kernels) are held to equality at the level the pinned path of the same mantissa width and mode chose.
  * The scaled kernels are NOT held to parity: the reference's algorithm keeps counting after an escape; what
    is asserted is the recorded offset histogram, a characterisation.
"""
import importlib.util
import os

import numpy as np
import pytest

import _oracle
import _truth
from fractalshark_amd import inputs

FX = _truth.fixture()["cases"]
SHALLOW = ["shallow_1e-6", "shallow_1e-12", "shallow_1e-20", "shallow_1e-28"]
# (the generated views whose samples all sit at the cap, or all on the real axis inside the set, carry nothing)
X2 = sorted(k for k in FX if k.startswith("x2_") and _truth.carries(k, "m53_po") and _truth.carries(k, "m53_lav2_gpustage"))
# the pinned pairs a CPU run cannot afford (104 s and 317 s of oracle for their 1920- and 7680-wide rows); the GPU tests render
# those frames
SLOW = {("view5_1920x1080", "m53_po"), ("view19_7680x4320", "m53_lav2_cpu")}
PINNED = [(c, k) for c in sorted(FX) for k in FX[c]["levels"] if (c, k) not in SLOW and FX[c]["levels"][k]["carries"]]
# pinned paths whose finest miss-free level holds fewer than 100 samples or 20 % of the case: nothing rests on them
NOT_CARRYING = {  # (case, pinned path): (finest miss-free level, samples stable at it)
    ("view11_64x36", "m24_po"): (None, 0),
    ("view11_64x36", "m24_bla"): (None, 0),
    ("view11_64x36", "m24_lav2_cpu"): (None, 0),
    ("view11_64x36", "m24_lav2_gpustage"): (None, 0),
    ("view19_7680x4320", "m24_bla"): (12, 0),
    ("view5_1920x1080", "m24_po"): (15, 16),
    ("view5_1920x1080", "m24_lav2_cpu"): (17, 36),
    ("view5_1920x1080", "m24_lav2_gpustage"): (17, 36),
    ("view5_3840x2160", "m24_lav2_cpu"): (17, 52),
    ("view5_3840x2160", "m24_lav2_gpustage"): (17, 52),
    ("view5_64x36", "m24_po"): (15, 20),
    ("view5_64x36", "m24_bla"): (17, 77),
    ("view5_64x36", "m24_lav2_cpu"): (17, 77),
    ("view5_64x36", "m24_lav2_gpustage"): (17, 77),
    ("view5_64x36", "m24_lav2_cpu_rc"): (15, 20),
    ("x2_c2_1e-14", "m53_bla"): (None, 0),
    ("x2_c2_1e-22", "m53_bla"): (None, 0),
    ("x2_c2_1e-31", "m53_bla"): (None, 0),
    ("x2_c2_1e-40", "m53_bla"): (None, 0),
}


def _gen():
    spec = importlib.util.spec_from_file_location("make_exact_counts", os.path.join(_truth.HERE, "golden", "make_exact_counts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _report(case, what, level, n_miss, n, share):
    print("exact-counts %-18s %-28s level 2^-%s  stable %4d (%4.1f %%)  misses %d" % (case.name, what, level, n, 100 * share, n_miss))


def _check(case, what, got, expected, R, level, mask=None):
    assert level is not None, (case.name, what, "no level of the ladder is free of misses for the pinned path of this width")
    n_miss, n, share = _truth.misses(case, got, expected, R, level, mask)
    _report(case, what, level, n_miss, n, share)
    assert n_miss == 0, (case.name, what, level, n_miss, n)


# ---- the counter itself
def test_counter_equals_python_integer_iteration(native_libs):
    """The second, independent implementation: Python integers on exact rationals, count for count."""
    c = _truth.Case("shallow_1e-12")
    bbox, F = c.view(inputs).bbox(), c.raw["frac_bits"]
    idx = np.arange(0, len(c.xs), 9)
    for R in (256, 4):
        E, _ = _truth.exact_counts(bbox, c.w, c.h, c.xs[idx], c.ys[idx], c.cap + 1, R, F, shifts=[])
        py = [_truth.python_exact_count(bbox, c.w, c.h, int(x), int(y), c.cap + 1, R, F) for x, y in zip(c.xs[idx], c.ys[idx])]
        assert E.tolist() == py
        assert E.tolist() == c.counts(R)[idx].tolist()
    # c = 2i (View 0's top row, middle column): |z_1|^2 = 4 exactly, z_2 = -4 + 2i -- at 4 on the first step, above it on the second
    v = inputs.View.builtin(0, 1024, 768)
    for inclusive, want in ((False, 2), (True, 1)):
        E, _ = _truth.exact_counts(v.bbox(), 1024, 768, [512], [0], 100, 4, 187, shifts=[], inclusive=inclusive)
        assert int(E[0]) == want == _truth.python_exact_count(v.bbox(), 1024, 768, 512, 0, 100, 4, 187, inclusive=inclusive)


def test_fixture_regenerates(native_libs):
    """One small case built again from its specification equals the committed entry (timings aside)."""
    gen = _gen()
    spec = [s for s in gen.cases() if s["name"] == "view0_70x37"][0]
    new = gen.build_case(spec, threads=8, log=lambda s: None)

    def strip(d):
        return {k: strip(v) for k, v in d.items() if "seconds" not in k} if isinstance(d, dict) else d
    assert strip(new) == strip(FX["view0_70x37"])


def test_fixture_holds_what_the_tests_rest_on():
    for name, c in FX.items():
        if c.get("attempt"):  # counts of a few samples with their wall time, no stability bits: nothing rests on it
            assert not c["levels"] and not c["ladder"] and c["R256"]["seconds"] > 0, name
            continue
        assert c["samples"] == len(c["rows"]) * len(c["columns"]) >= 200, name
        assert c["rows"][0] == 0 and c["rows"][-1] == c["height"] - 1 and c["columns"][-1] == c["width"] - 1, name
        for key, lv in c["levels"].items():
            assert lv["level"] in c["ladder"] or not lv["carries"], (name, key, lv)


def test_which_pinned_paths_carry_no_comparison():
    """The floors are not lowered: where a pinned path's stable set is too small the path is left out, and this list says where.
    HDRFloat<float> at View 5's depth (1e-100 wide, 8e4 steps) and deeper (Views 11 and 19: no miss-free level at all); and the
    BLA function on the third generated centre, where it counts the
    escaping step when a BLA skip lands on it (121 for an exact 120 on every sample: level None) -- see DESIGN.md 2.2."""
    got = {(c, k): (FX[c]["levels"][k]["level"], FX[c]["levels"][k]["stable"]) for c in sorted(FX) for k in FX[c]["levels"]
           if not FX[c]["levels"][k]["carries"]}
    assert got == NOT_CARRYING


# ---- pinned paths: they chose the levels, and must hold them
@pytest.mark.parametrize("name,key", PINNED)
def test_pinned_oracle_paths_equal_exact_counts(native_libs, name, key):
    c = _truth.Case(name)
    v = c.view(inputs)
    render = _truth.pinned_paths(v, c.cap, [key])[key]
    got = _truth.sample_rows(render, c.w, c.xs, c.ys)
    R = 4 if "direct" in key else 256
    _check(c, key, got, _truth.expect_minus_one(c.counts(R), c.cap), R, c.levels[key]["level"])


@pytest.mark.parametrize("name", SHALLOW + ["view5_64x36"])
def test_plain_double_bla_equals_exact_counts(native_libs, name):
    """Cpu64PerturbedBLA (double, golden CRC f201db00ade569fc), with and without its table, at the HDRFloat<double> levels."""
    c = _truth.Case(name)
    v = c.view(inputs)
    ob = inputs.OrbitF64(v)
    for use_bla, key in ((False, "m53_po"), (True, "m53_bla")):
        got = c.sample(_oracle.bla_f64(v, ob, use_bla=use_bla))
        _check(c, "bla_f64 " + key, got, _truth.expect_minus_one(c.counts(256), c.cap), 256, c.levels[key]["level"])


# ---- unpinned restatements
def _x2_inputs(v):
    o = inputs.Orbit(v, is64=True)
    la = inputs.LATable(o, use_small_exponents=True)
    return inputs.Orbit2x32(o), inputs.LATable2x32(la)


@pytest.mark.parametrize("name", X2 + SHALLOW + ["view5_64x36"])
def test_hdr2x32_lav2_restatement_equals_exact_counts(native_libs, name):
    """mandel_1xHDR_float_perturb_lav2<HDRFloat<CudaDblflt>> (oracle/gpu_ref_2x32.cpp).  Rule: the kernel steps, then counts the
    step while compareToBothPositiveReducedTemplate<256>(|z|^2) < 0 (LAKernel.cuh:133-235); that template compares the
    exponent with 1 (HDRFloat.h:1169-1184), so the bailout is at 4, not 256: expected = min(E_4 - 1, N) (that it stops AT 4: the boundary test below).  48-bit
    mantissas: the HDRFloat<double> levels, LAv2 Full at Case.approx_level, PO at the PO level."""
    c = _truth.Case(name)
    v = c.view(inputs)
    o2, la2 = _x2_inputs(v)
    E = c.counts(4)
    full = c.sample(_oracle.gpu_lav2_2x32(v, o2, la2, mode=0, n_iterations=c.cap))
    rec = c.raw.get("characterised", {}).get("hdr2x32_full")
    if rec:  # an escaping reference orbit: LA steps pass the bailout at 4 (make_exact_counts.hdr2x32_escaping_orbit_record)
        assert _truth.offsets(c, full, _truth.expect_minus_one(E, c.cap), 4, rec["level"]) == rec["offsets"]
    else:
        _check(c, "gpu_lav2_2x32 full", full, _truth.expect_minus_one(E, c.cap), 4, c.approx_level("m53"))
    n = 4000 if name.startswith("x2_") else c.cap  # the cap test_2x32_generated_views_* renders PO with
    if name != "view5_64x36":  # (8e4 double-float steps per pixel there: the GPU test's)
        po = c.sample(_oracle.gpu_lav2_2x32(v, o2, None, mode=1, n_iterations=n))
        _check(c, "gpu_lav2_2x32 po", po, _truth.expect_minus_one(E, n), 4, c.levels["m53_po"]["level"])


@pytest.mark.parametrize("kind", ["f32", "f64", "2x32"])
@pytest.mark.parametrize("name", SHALLOW)
def test_plain_lav2_restatement_equals_exact_counts(native_libs, name, kind):
    """mandel_1xHDR_float_perturb_lav2<T, T> for T = float / double / CudaDblflt (oracle/gpu_ref_plain.cpp).  Rule: step, then
    count while |z|^2 < 256 (`one < T(256)`, HDRFloat.h:1536-1586; LAKernel.cuh:133-235): expected = min(E_256 - 1, N), E_256
    (that it stops AT 256: the boundary test below).  float at the HDRFloat<float> levels, double and CudaDblflt (48 bits) at the
    HDRFloat<double> ones; Full at Case.approx_level.  Where CudaDblflt's operator<= sends most pixels through AT outside its
    radius, Full is left out (make_exact_counts.plain_2x32_at_record; test_2x32_at_validity_* covers the cause)."""
    c = _truth.Case(name)
    v = c.view(inputs)
    pin = inputs.PlainInputs(v, kind)
    m = "m24" if kind == "f32" else "m53"
    want = _truth.expect_minus_one(c.counts(256), c.cap)
    for mode, level in ((0, c.approx_level(m)), (1, c.levels[m + "_po"]["level"])):
        if kind == "2x32" and mode == 0 and "plain_2x32_full" in c.raw.get("excluded", {}):
            continue  # AT taken outside its radius on every pixel (the reference's operator<=): not an exact-count path here
        got = c.sample(_oracle.gpu_lav2_plain(v, pin, mode=mode))
        _check(c, "gpu_lav2_plain %s mode %d" % (kind, mode), got, want, 256, level)


@pytest.mark.parametrize("kind,ip", [("1x32", 1), ("1x32", 4), ("1x32", 16), ("2x32", 1), ("2x32", 8), ("2x64", 1), ("4x32", 1),
                                     ("4x64", 1)])
@pytest.mark.parametrize("name", ["view0_70x37", "view0_1024x768"])
def test_low_precision_direct_restatements_equal_exact_counts(native_libs, name, kind, ip):
    """The five direct kernels without a CPU twin (oracle/gpu_ref_lp.cpp, gpu_ref_qd.cpp): rule and row shift in tests/_truth.py
    (output row r is sample row r + 1, so the samples of row 0 have no output row).  float at CpuHDR32's level, the wider types at
    Cpu64's."""
    c = _truth.Case(name)
    v = c.view(inputs)
    got = _truth.sample_rows(lambda y0, y1: _oracle.gpu_direct_lp(v, kind, ip, rows=(y0, y1), n_iterations=c.cap), c.w,
                             c.xs[c.ys > 0], c.ys[c.ys > 0] - 1)
    full = np.zeros(len(c.xs), np.int64)
    full[c.ys > 0] = got
    _check(c, "gpu_direct_lp %s ip %d" % (kind, ip), full, _truth.expect_lp_direct(c.counts(4), c.cap, ip, kind), 4,
           c.levels["m24_direct" if kind == "1x32" else "m53_direct"]["level"], mask=c.ys > 0)


# ---- strict or inclusive bailout, on samples where |z_n|^2 == 4 exactly
def test_direct_paths_bail_strictly_or_inclusively_as_the_reference_writes_it(native_libs):
    """CalcCpuHDR tests `> 4` (Fractal.cpp:2096-2206): c = 2i counts to 1, c = -2 to the cap.  The low-precision CUDA kernels loop
    `while (|z|^2 < 4 ...)` (LowPrecisionKernels.cuh:171-290, :384-555, :682-777), so they stop AT 4: both samples count 1 (rounded
    up to iteration_precision); the quad kernels loop `<= 4.0` (:5-75, :77-140) and count 2 and the cap.  tests/_truth.py, BOUNDARY."""
    v = _truth.boundary_view(inputs)
    strict, incl = _truth.boundary_counts(v, False), _truth.boundary_counts(v, True)
    assert strict.tolist() == [2, 0] and incl.tolist() == [1, 1]
    cap = _truth.BOUNDARY_CAP
    for name, frame in (("direct_f64", _oracle.direct_f64(v)), ("direct_hdr32", _oracle.direct_hdr(v, False)),
                        ("direct_hdr64", _oracle.direct_hdr(v, True))):
        got = [int(frame[y, x]) for x, y in _truth.BOUNDARY_SAMPLES]
        assert got == _truth.expect_minus_one(strict, cap).tolist(), name
    for kind, ip in (("1x32", 1), ("1x32", 4), ("1x32", 16), ("2x32", 1), ("2x32", 8), ("2x64", 1), ("4x32", 1), ("4x64", 1)):
        frame = _oracle.gpu_direct_lp(v, kind, ip)
        got = [int(frame[r, x]) for x, r in _truth.BOUNDARY_SAMPLES_LP]
        mine, other = (incl, strict) if _truth.LP_BAILS_AT_EQUALITY[kind] else (strict, incl)
        assert got == _truth.expect_lp_direct(mine, cap, ip, kind).tolist(), (kind, ip)
        assert got != _truth.expect_lp_direct(other, cap, ip, kind).tolist(), (kind, ip)


def test_perturbation_paths_bail_strictly_or_inclusively_as_the_reference_writes_it(native_libs):
    """The reference point itself (delta c = 0; tests/_truth.py, BOUNDARY).  c = -16: the CPU functions test `> 256`
    (Fractal.cpp:2329, :2444, :2660) and count 1; the plain-type CUDA kernel counts while `|z|^2 < 256` (LAKernel.cuh:133-235,
    HDRFloat.h:1536-1586) and counts 0.  c = -2: the HDRFloat<CudaDblflt> kernel, whose compareToBothPositiveReducedTemplate<256>
    bails from 4 on (HDRFloat.h:1169-1184), counts 0 where a bailout above 4 would never trigger."""
    cap, (x, y) = _truth.BOUNDARY_CAP, _truth.BOUNDARY_CENTRE
    v = _truth.boundary_view(inputs, _truth.BOUNDARY_BBOX_256)
    strict, incl = _truth.boundary_centre_count(v, 256, False), _truth.boundary_centre_count(v, 256, True)
    assert (strict.tolist(), incl.tolist()) == ([2], [1])
    want_strict, want_incl = int(_truth.expect_minus_one(strict, cap)[0]), int(_truth.expect_minus_one(incl, cap)[0])
    for key, render in _truth.pinned_paths(v, cap, _truth.PERTURB_KEYS).items():
        assert int(render(y, y + 1)[y, x]) == want_strict != want_incl, key
    for use_bla in (False, True):
        assert int(_oracle.bla_f64(v, inputs.OrbitF64(v), use_bla=use_bla)[y, x]) == want_strict
    for kind in ("f32", "f64", "2x32"):
        for mode in (0, 1):
            assert int(_oracle.gpu_lav2_plain(v, inputs.PlainInputs(v, kind), mode=mode)[y, x]) == want_incl, (kind, mode)
    v = _truth.boundary_view(inputs, _truth.BOUNDARY_BBOX_CENTRE_4)
    strict, incl = _truth.boundary_centre_count(v, 4, False), _truth.boundary_centre_count(v, 4, True)
    assert (strict.tolist(), incl.tolist()) == ([0], [1])
    o2, la2 = _x2_inputs(v)
    for table, mode in ((la2, 0), (None, 1)):
        got = int(_oracle.gpu_lav2_2x32(v, o2, table, mode=mode)[y, x])
        assert got == int(_truth.expect_minus_one(incl, cap)[0]) != int(_truth.expect_minus_one(strict, cap)[0]), mode


# ---- scaled kernels: a characterisation, not parity
@pytest.mark.parametrize("which", ["hdr32", "f64"])
@pytest.mark.parametrize("name", [n for n in SHALLOW + ["view5_64x36", "view3_64x36"] if "scaled" in FX[n]])
def test_scaled_restatement_reproduces_its_recorded_offsets(native_libs, name, which):
    """mandel_1x_float_perturb_scaled (ScaledKernels.cuh:3-239) is not an exact-count algorithm: `test1a` (:111) is not gated on
    `zn_size_OK`, so an escaped z with |z|^2 < |delta|^2 rebases and goes on counting, and a `bad` entry bails at |z|^2 >= 4
    (:200).  DESIGN.md 2.2.  The fixture records, from the restatement, the histogram of output - min(E_256 - 1, N) on the
    samples stable at the HDRFloat<float> PO level; this asserts the restatement still produces it."""
    c = _truth.Case(name)
    v = c.view(inputs)
    rec = c.raw["scaled"][which]
    assert _truth.scaled_offsets(c, v, which, rec["level"]) == rec["offsets"]
