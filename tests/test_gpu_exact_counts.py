"""Every kernel family, through the C ABI, against exact escape counts (tests/golden/exact_counts.json, tests/_truth.py).

The frames are rendered at the fixture's sizes -- the BASELINE frames for C1, C2, C3 and C5 -- and only the sampled pixels are
read back and compared, under the same rule as tests/test_exact_counts.py: equality with the value derived from the exact count,
on the samples stable at the level the reference-pinned oracle of the same mantissa width and mode chose.  Nothing here reads
the oracle's output for the comparison (the scaled kernels' recorded characterisation aside), and nothing reads a reference tree:
the fixture and the product only.
"""
import numpy as np
import pytest

import _truth
from fractalshark_amd import (GPURenderer, LAV2_FULL, LAV2_PO, PARITY_CPU, PARITY_CPU_GPUSTAGE, T_2X32, T_2X64, T_4X32, T_4X64,
                              T_F32, T_F64, T_HDR2X32, T_HDR32, T_HDR64, inputs)

pytestmark = pytest.mark.gpu

FX = _truth.fixture()["cases"]
SHALLOW = ["shallow_1e-6", "shallow_1e-12", "shallow_1e-20", "shallow_1e-28"]
# (the generated views whose samples all sit at the cap, or all on the real axis inside the set, carry nothing)
X2 = sorted(k for k in FX if k.startswith("x2_") and _truth.carries(k, "m53_po") and _truth.carries(k, "m53_lav2_gpustage"))


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.set_kernel_variant(0)
    r.close()


def _pairs(co):
    return [(float(c["m"]), int(c["e"])) for c in co]


def _read(r, n):
    out = r.new_iter_buffer()
    assert r.RenderCurrent(n, out) == 0
    assert r.SyncComputeStream() == 0
    return out


def _check(case, what, frame, expected, R, level, row_shift=0):
    assert level is not None, (case.name, what)
    keep = case.ys >= row_shift  # samples the kernel has an output row for; the others leave the stable set
    got = np.zeros(len(case.xs), np.int64)
    got[keep] = np.asarray(frame)[case.ys[keep] - row_shift, case.xs[keep]].astype(np.int64)
    n_miss, n, share = _truth.misses(case, got, expected, R, level, mask=keep)
    print("exact-counts %-18s %-30s level 2^-%s  stable %4d (%4.1f %%)  misses %d" % (case.name, what, level, n, 100 * share, n_miss))
    assert n_miss == 0, (case.name, what, level, n_miss, n)


def _lav2(r, c, v, ob, la, mode, parity, n=None, iter_bytes=4):
    n = c.cap if n is None else n
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False, iter_bytes=iter_bytes) == 0
    table = inputs.LATableU64(la) if iter_bytes == 8 and la is not None else la
    assert r.InitializePerturb(1, ob, 0, None, table, iter_bytes=iter_bytes) == 0
    assert r.ClearMemory() == 0
    T = T_HDR64 if ob.is64 else T_HDR32
    assert r.RenderPerturbLAv2(None, None, None, *_pairs(v.coords_perturb(ob)), n, T=T, Mode=mode, parity=parity) == 0
    assert r.SyncComputeStream() == 0
    return _read(r, n)


# ---- LAv2, HDRFloat<float> and HDRFloat<double>: Full in both stage-test directions, perturbation only
def _carrying(pairs, suffix):
    """(case, is64) pairs whose pinned path of that width chose a level that meets the floors (tests/_truth.carries)."""
    return [(n, w) for n, w in pairs if _truth.carries(n, ("m53" if w else "m24") + suffix)]


@pytest.mark.parametrize("name,is64", _carrying([("view19_7680x4320", True), ("view11_64x36", True), ("view11_64x36", False),
                                                 ("view5_3840x2160", False), ("view5_3840x2160", True), ("view5_64x36", False),
                                                 ("view5_64x36", True), ("view3_64x36", False), ("view3_64x36", True),
                                                 ("view9_64x36", True), ("shallow_1e-20", False), ("shallow_1e-20", True)],
                                                "_lav2_gpustage"))
def test_lav2_full_equals_exact_counts(renderer, native_libs, name, is64):
    c = _truth.Case(name)
    v = c.view(inputs)
    ob = inputs.Orbit(v, is64=is64)
    la = inputs.LATable(ob)
    want = _truth.expect_minus_one(c.counts(256), c.cap)
    m = "m53" if is64 else "m24"
    for parity, key in ((PARITY_CPU, m + "_lav2_cpu"), (PARITY_CPU_GPUSTAGE, m + "_lav2_gpustage")):
        # (View 19 in the CPU's stage-test direction is perturbation steps almost throughout: 317 s of oracle for ten rows, and
        # 2.7 million HDRFloat<double> steps for each of 33 million pixels here; the GPU direction is the one rendered)
        if _truth.carries(name, key) and (name, key) != ("view19_7680x4320", "m53_lav2_cpu"):
            _check(c, "lav2 full " + key, _lav2(renderer, c, v, ob, la, LAV2_FULL, parity), want, 256, c.levels[key]["level"])


@pytest.mark.parametrize("name,is64,literal", [(n, w, lit) for n, w, lit in [
    ("view11_64x36", True, False), ("view11_64x36", False, False), ("view5_1920x1080", False, False), ("view5_1920x1080", True, False), ("view5_64x36", False, True), ("view5_64x36", True, False),
    ("view3_64x36", False, True), ("shallow_1e-28", False, False), ("shallow_1e-28", False, True), ("shallow_1e-28", True, False)]
    if _truth.carries(n, ("m53" if w else "m24") + "_po")])
def test_perturbation_only_equals_exact_counts(renderer, native_libs, name, is64, literal):
    """C2's frame (in the type whose level carries it), and the literal transcription of the loop at a small one."""
    c = _truth.Case(name)
    v = c.view(inputs)
    ob = inputs.Orbit(v, is64=is64)
    try:
        assert renderer.set_kernel_variant(literal=literal) == 0
        out = _lav2(renderer, c, v, ob, inputs.LATable(ob), LAV2_PO, PARITY_CPU)
    finally:
        renderer.set_kernel_variant(literal=False)
    key = ("m53" if is64 else "m24") + "_po"
    _check(c, "lav2 po " + key + (" literal" if literal else ""), out, _truth.expect_minus_one(c.counts(256), c.cap), 256,
           c.levels[key]["level"])


@pytest.mark.parametrize("is64", [w for w in (False, True) if _truth.carries("view5_64x36", ("m53" if w else "m24") + "_lav2_cpu_rc")])
def test_in_kernel_decompression_equals_exact_counts(renderer, native_libs, is64):
    """GpuHDRx32 / x64 PerturbedRCLAv2: the waypoints of a SimpleCompression orbit, expanded on the device."""
    c = _truth.Case("view5_64x36")
    v = c.view(inputs)
    ob = inputs.Orbit(v, is64=is64, compression_exp=20)
    assert ob.compressed
    key = ("m53" if is64 else "m24") + "_lav2_cpu_rc"
    out = _lav2(renderer, c, v, ob, inputs.LATable(ob), LAV2_FULL, PARITY_CPU)
    _check(c, "lav2 full rc " + key, out, _truth.expect_minus_one(c.counts(256), c.cap), 256, c.levels[key]["level"])


def test_uint64_itertype_equals_exact_counts(renderer, native_libs):
    c = _truth.Case("view3_64x36")
    v = c.view(inputs)
    ob = inputs.Orbit(v)
    try:
        out = _lav2(renderer, c, v, ob, inputs.LATable(ob), LAV2_FULL, PARITY_CPU_GPUSTAGE, iter_bytes=8)
    finally:
        assert renderer.InitializeMemory(64, 36, 1, None, 0, 0, 0, False, iter_bytes=4) == 0
    assert out.dtype == np.uint64 and _truth.carries(c.name, "m24_lav2_gpustage")
    _check(c, "lav2 full uint64", out, _truth.expect_minus_one(c.counts(256), c.cap), 256, c.levels["m24_lav2_gpustage"]["level"])


# ---- BLA: HDRFloat<float>, HDRFloat<double>, double
@pytest.mark.parametrize("name,is64", _carrying([("view19_7680x4320", False), ("view19_7680x4320", True), ("view11_64x36", True),
                                                 ("view11_64x36", False), ("view5_64x36", False), ("view5_64x36", True),
                                                 ("view3_64x36", False), ("view3_64x36", True), ("view9_64x36", True), ("shallow_1e-12", False),
                                                 ("shallow_1e-12", True)], "_bla"))
def test_bla_equals_exact_counts(renderer, native_libs, name, is64):
    c = _truth.Case(name)
    v = c.view(inputs)
    ob = inputs.Orbit(v, is64=is64)
    bla = inputs.BLATable(ob)
    r = renderer
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0
    assert r.ClearMemory() == 0
    assert r.RenderPerturbBLA(None, ob, bla, None, None, *_pairs(v.coords_perturb(ob)), c.cap) == 0
    key = ("m53" if is64 else "m24") + "_bla"
    _check(c, "bla " + key, _read(r, c.cap), _truth.expect_minus_one(c.counts(256), c.cap), 256, c.levels[key]["level"])


@pytest.mark.parametrize("name", SHALLOW + ["view5_64x36"])
def test_plain_double_bla_equals_exact_counts(renderer, native_libs, name):
    c = _truth.Case(name)
    v = c.view(inputs)
    ob = inputs.OrbitF64(v)
    r, lib = renderer, renderer._lib
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0
    assert lib.fs_upload_orbit(r._h, 0, T_F64, 4, ob.data_ptr, ob.count, ob.count, ob.period) == 0
    co = ob.coords()
    for use_bla, key in ((True, "m53_bla"), (False, "m53_po")):
        if use_bla:
            assert lib.fs_upload_bla(r._h, T_F64, ob.level_ptrs, ob.level_sizes, ob.num_levels, ob.lm2) == 0
        else:
            assert lib.fs_upload_bla(r._h, T_F64, None, None, 0, 0) == 0
        assert r.ClearMemory() == 0
        assert lib.fs_render_bla(r._h, T_F64, co.ctypes.data, c.cap) == 0
        _check(c, "bla f64 " + key, _read(r, c.cap), _truth.expect_minus_one(c.counts(256), c.cap), 256, c.levels[key]["level"])


# ---- direct kernels (C1 at its BASELINE size)
@pytest.mark.parametrize("name", ["view0_1024x768", "view0_70x37"])
def test_direct_kernels_equal_exact_counts(renderer, native_libs, name):
    """Rules and the low-precision kernels' row shift: tests/_truth.py."""
    c = _truth.Case(name)
    v = c.view(inputs)
    r = renderer
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0
    want = _truth.expect_minus_one(c.counts(4), c.cap)
    dx, dy, minx, maxy = v.coords_direct_f64()
    assert r.ClearMemory() == 0
    assert r.Render(None, minx, maxy, dx, dy, c.cap, T=T_F64) == 0
    _check(c, "direct f64", _read(r, c.cap), want, 4, c.levels["m53_direct"]["level"])
    for is64, key in ((False, "m24_direct"), (True, "m53_direct_hdr")):
        dx, dy, minx, maxy = _pairs(v.coords_direct_hdr(is64))
        assert r.ClearMemory() == 0
        assert r.Render(None, minx, maxy, dx, dy, c.cap, T=T_HDR64 if is64 else T_HDR32) == 0
        _check(c, "direct hdr " + key, _read(r, c.cap), want, 4, c.levels[key]["level"])
    E = c.counts(4)
    for kind, ip, T in (("1x32", 1, T_F32), ("1x32", 4, T_F32), ("1x32", 16, T_F32), ("2x32", 1, T_2X32), ("2x32", 8, T_2X32),
                        ("2x64", 1, T_2X64), ("4x32", 1, T_4X32), ("4x64", 1, T_4X64)):
        assert r.ClearMemory() == 0
        assert r.RenderLowPrecision(None, v.coords_direct_lp(kind), c.cap, ip, T=T) == 0
        _check(c, "direct %s ip %d" % (kind, ip), _read(r, c.cap), _truth.expect_lp_direct(E, c.cap, ip, kind), 4,
               c.levels["m24_direct" if kind == "1x32" else "m53_direct"]["level"], row_shift=1)


def test_direct_kernels_bail_strictly_or_inclusively_as_the_reference_writes_it(renderer, native_libs):
    """c = 2i and c = -2, where |z_n|^2 == 4 exactly (tests/_truth.py, BOUNDARY): the CPU-twin and quad kernels test `> 4`, the
    other low-precision ones stop at 4."""
    v = _truth.boundary_view(inputs)
    strict, incl = _truth.boundary_counts(v, False), _truth.boundary_counts(v, True)
    cap, n, r = _truth.BOUNDARY_CAP, _truth.BOUNDARY_SIZE, renderer
    assert r.InitializeMemory(n, n, 1, None, 0, 0, 0, False) == 0
    frames = []
    dx, dy, minx, maxy = v.coords_direct_f64()
    assert r.ClearMemory() == 0 and r.Render(None, minx, maxy, dx, dy, cap, T=T_F64) == 0
    frames.append(("f64", _read(r, cap)))
    for is64 in (False, True):
        dx, dy, minx, maxy = _pairs(v.coords_direct_hdr(is64))
        assert r.ClearMemory() == 0 and r.Render(None, minx, maxy, dx, dy, cap, T=T_HDR64 if is64 else T_HDR32) == 0
        frames.append(("hdr64" if is64 else "hdr32", _read(r, cap)))
    for name, frame in frames:
        assert [int(frame[y, x]) for x, y in _truth.BOUNDARY_SAMPLES] == _truth.expect_minus_one(strict, cap).tolist(), name
    for kind, ip, T in (("1x32", 1, T_F32), ("1x32", 4, T_F32), ("1x32", 16, T_F32), ("2x32", 1, T_2X32), ("2x32", 8, T_2X32),
                        ("2x64", 1, T_2X64), ("4x32", 1, T_4X32), ("4x64", 1, T_4X64)):
        assert r.ClearMemory() == 0 and r.RenderLowPrecision(None, v.coords_direct_lp(kind), cap, ip, T=T) == 0
        frame = _read(r, cap)
        got = [int(frame[row, x]) for x, row in _truth.BOUNDARY_SAMPLES_LP]
        mine, other = (incl, strict) if _truth.LP_BAILS_AT_EQUALITY[kind] else (strict, incl)
        assert got == _truth.expect_lp_direct(mine, cap, ip, kind).tolist(), (kind, ip)
        assert got != _truth.expect_lp_direct(other, cap, ip, kind).tolist(), (kind, ip)


def test_perturbation_kernels_bail_strictly_or_inclusively_as_the_reference_writes_it(renderer, native_libs):
    """The reference point itself, delta c = 0 (tests/_truth.py, BOUNDARY; rules: the CPU test of the same name)."""
    cap, n, (x, y), r = _truth.BOUNDARY_CAP, _truth.BOUNDARY_SIZE, _truth.BOUNDARY_CENTRE, renderer
    v = _truth.boundary_view(inputs, _truth.BOUNDARY_BBOX_256)
    strict, incl = _truth.boundary_centre_count(v, 256, False), _truth.boundary_centre_count(v, 256, True)
    want_strict, want_incl = int(_truth.expect_minus_one(strict, cap)[0]), int(_truth.expect_minus_one(incl, cap)[0])
    assert (want_strict, want_incl) == (1, 0)

    class Frame:
        w = h = n
    Frame.cap = cap
    for is64 in (False, True):
        ob = inputs.Orbit(v, is64=is64)
        la = inputs.LATable(ob)
        for mode, parity in ((LAV2_FULL, PARITY_CPU), (LAV2_FULL, PARITY_CPU_GPUSTAGE), (LAV2_PO, PARITY_CPU)):
            assert int(_lav2(r, Frame, v, ob, la, mode, parity)[y, x]) == want_strict, (is64, mode, parity)
        assert r.ClearMemory() == 0
        assert r.RenderPerturbBLA(None, ob, inputs.BLATable(ob), None, None, *_pairs(v.coords_perturb(ob)), cap) == 0
        assert int(_read(r, cap)[y, x]) == want_strict, ("bla", is64)
    for kind in ("f32", "f64", "2x32"):
        pin = inputs.PlainInputs(v, kind)
        for mode in (LAV2_FULL, LAV2_PO):
            assert r.InitializeMemory(n, n, 1, None, 0, 0, 0, False) == 0
            assert r.InitializePerturbPlain(0, pin) == 0
            assert r.ClearMemory() == 0
            assert r.RenderPerturbLAv2Plain(pin, cap, Mode=mode) == 0
            assert r.SyncComputeStream() == 0
            assert int(_read(r, cap)[y, x]) == want_incl, (kind, mode)
    v = _truth.boundary_view(inputs, _truth.BOUNDARY_BBOX_CENTRE_4)
    strict, incl = _truth.boundary_centre_count(v, 4, False), _truth.boundary_centre_count(v, 4, True)
    o = inputs.Orbit(v, is64=True)
    o2, la2 = inputs.Orbit2x32(o), inputs.LATable2x32(inputs.LATable(o, use_small_exponents=True))
    co = [(float(t["head"]), float(t["tail"]), int(t["e"])) for t in v.coords_perturb_2x32(o2)]
    for mode, table in ((LAV2_FULL, la2), (LAV2_PO, None)):
        assert r.InitializeMemory(n, n, 1, None, 0, 0, 0, False) == 0
        assert r.InitializePerturb(0, o2, 0, None, table) == 0
        assert r.ClearMemory() == 0
        assert r.RenderPerturbLAv2(None, None, None, *co, cap, T=T_HDR2X32, Mode=mode) == 0
        assert r.SyncComputeStream() == 0
        got = int(_read(r, cap)[y, x])
        assert got == int(_truth.expect_minus_one(incl, cap)[0]) != int(_truth.expect_minus_one(strict, cap)[0]), mode


# ---- HDRFloat<CudaDblflt> LAv2 (C4 "as specified"'s arithmetic): Full and perturbation only
@pytest.mark.parametrize("name", X2 + SHALLOW + ["view5_64x36"])
def test_hdr2x32_lav2_equals_exact_counts(renderer, native_libs, name):
    """Rule: min(E_4 - 1, N) (tests/test_exact_counts.py, the restatement's test)."""
    c = _truth.Case(name)
    v = c.view(inputs)
    o = inputs.Orbit(v, is64=True)
    o2, la2 = inputs.Orbit2x32(o), inputs.LATable2x32(inputs.LATable(o, use_small_exponents=True))
    r = renderer
    E = c.counts(4)
    co = [(float(t["head"]), float(t["tail"]), int(t["e"])) for t in v.coords_perturb_2x32(o2)]
    n_po = 4000 if name.startswith("x2_") else c.cap
    for mode, table, n, level in ((LAV2_FULL, la2, c.cap, c.approx_level("m53")), (LAV2_PO, None, n_po, c.levels["m53_po"]["level"])):
        assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0
        assert r.InitializePerturb(0, o2, 0, None, table) == 0
        assert r.ClearMemory() == 0
        assert r.RenderPerturbLAv2(None, None, None, *co, n, T=T_HDR2X32, Mode=mode) == 0
        assert r.SyncComputeStream() == 0
        out = _read(r, n)
        rec = c.raw.get("characterised", {}).get("hdr2x32_full")
        if mode == LAV2_FULL and rec:  # recorded characterisation (an escaping reference orbit, tests/test_exact_counts.py)
            assert _truth.offsets(c, c.sample(out), _truth.expect_minus_one(E, n), 4, rec["level"]) == rec["offsets"]
        else:
            _check(c, "hdr2x32 lav2 mode %d" % mode, out, _truth.expect_minus_one(E, n), 4, level)


# ---- plain-type LAv2: float, double, CudaDblflt
@pytest.mark.parametrize("kind", ["f32", "f64", "2x32"])
@pytest.mark.parametrize("name", SHALLOW)
def test_plain_lav2_equals_exact_counts(renderer, native_libs, name, kind):
    """Rule: min(E_256 - 1, N) (tests/test_exact_counts.py, the restatement's test)."""
    c = _truth.Case(name)
    v = c.view(inputs)
    pin = inputs.PlainInputs(v, kind)
    r = renderer
    m = "m24" if kind == "f32" else "m53"
    want = _truth.expect_minus_one(c.counts(256), c.cap)
    for mode, level in ((LAV2_FULL, c.approx_level(m)), (LAV2_PO, c.levels[m + "_po"]["level"])):
        assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0
        assert r.InitializePerturbPlain(0, pin) == 0
        assert r.ClearMemory() == 0
        assert r.RenderPerturbLAv2Plain(pin, c.cap, Mode=mode) == 0
        assert r.SyncComputeStream() == 0
        out = _read(r, c.cap)
        if kind == "2x32" and mode == LAV2_FULL and "plain_2x32_full" in c.raw.get("excluded", {}):
            continue  # not an exact-count path on this case (tests/test_exact_counts.py); the render above still has to succeed
        _check(c, "plain lav2 %s mode %d" % (kind, mode), out, want, 256, level)


# ---- scaled kernels: the recorded characterisation (not parity), tuned and literal variant
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("which", ["hdr32", "f64"])
@pytest.mark.parametrize("name", [n for n in SHALLOW + ["view5_64x36", "view3_64x36"] if "scaled" in FX[n]])
def test_scaled_kernels_reproduce_the_recorded_offsets(renderer, native_libs, name, which, variant):
    c = _truth.Case(name)
    v = c.view(inputs)
    r = renderer
    assert r.InitializeMemory(c.w, c.h, 1, None, 0, 0, 0, False) == 0
    try:
        assert r.set_kernel_variant(variant) == 0
        assert r.ClearMemory() == 0
        if which == "hdr32":
            ob = inputs.Orbit(v)
            assert r.RenderPerturbBLAScaled(None, ob, ob, None, None, *_pairs(v.coords_perturb(ob)), c.cap) == 0
        else:
            ob = inputs.OrbitF64(v)
            co = ob.coords()
            assert r.RenderPerturbBLAScaled(None, ob, ob, None, None, co[0], co[1], co[2], co[3], c.cap, T=T_F64) == 0
        out = _read(r, c.cap)
    finally:
        r.set_kernel_variant(0)
    rec = c.raw["scaled"][which]
    assert _truth.scaled_offsets(c, v, which, rec["level"], render=out) == rec["offsets"]
