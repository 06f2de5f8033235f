"""GPU: what the kernel launchers select for a step-counting launch (fs_enable_step_count), family by family.

Every launcher picks one instantiation of its kernel from run-time switches: the mode, step counting, 64-bit counters, the
waypoint-resident orbit, the variant.  tests/test_gpu_wide_counters.py pins the 64-bit selection; the counting one was pinned for
the tuned HDRFloat<float> LAv2 kernel, the fast HDRFloat<double> one, the scaled kernels and the perturbation-only kernel.  Here,
for every other family: the frame of a counting launch equals the frame of a plain one, the counting launch saw every pixel of
the frame once (word 3 of fs_read_step_count), and it counted perturbation steps where the family takes any (word 2).  And the
two cases in which no counters exist -- 64-bit counters, a plain or 2x32 kernel on a waypoint-resident orbit -- are refused by
fs_read_step_count instead of read as zeros.

70 x 37: neither side is a multiple of a tile (8 x 8), a tile row (32) or a wave (64); inputs as in test_gpu_wide_counters.py."""
import ctypes as C

import numpy as np
import pytest

from fractalshark_amd import (GPURenderer, LAV2_FULL, LAV2_LAO, LAV2_PO, PARITY_CPU, PARITY_CPU_GPUSTAGE, T_2X32, T_2X64, T_4X32,
                              T_4X64, T_F32, T_F64, T_HDR2X32, T_HDR32, T_HDR64, inputs)

pytestmark = pytest.mark.gpu
W, H = 70, 37
FS_ERR_UNSUPPORTED = 10100  # include/fsmi355.h
# PO with CPU parity is served by the perturbation-only kernel (fs_render_bla), so the LAv2 kernels' own PO runs with the other one
MODES = ((LAV2_FULL, PARITY_CPU), (LAV2_PO, PARITY_CPU_GPUSTAGE), (LAV2_LAO, PARITY_CPU_GPUSTAGE))


def _pairs(co):
    return [(float(c["m"]), int(c["e"])) for c in co]


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.enable_step_count(False)
    r.set_compressed_orbit_mode(False)
    r.set_kernel_variant(0)
    r.close()


@pytest.fixture(scope="module")
def v5(native_libs):
    """View 5 at 70 x 37 with its HDRFloat<float | double> orbits and tables, plain and compressed."""
    v = inputs.View.builtin(5, W, H)
    d = {"v": v}
    for is64 in (False, True):
        ob = inputs.Orbit(v, is64=is64)
        oc = inputs.Orbit(v, is64=is64, compression_exp=20)
        d[is64] = (ob, inputs.LATable(ob), oc, inputs.LATable(oc))
    return d


def _frame(r, n):
    out = r.new_iter_buffer()
    assert r.RenderCurrent(n, out) == 0
    assert r.SyncComputeStream() == 0
    return out


def _counted(r, setup, render, n, takes_steps, what):
    """Renders once without and once with step counting and checks the three properties of the module's docstring."""
    assert r.InitializeMemory(W, H, 1, None, 0, 0, 0, False) == 0
    assert setup() == 0
    frames = []
    try:
        for on in (False, True):
            r.enable_step_count(on)
            assert r.ClearMemory() == 0
            assert render() == 0
            frames.append(_frame(r, n))
        st = r.read_step_count()
    finally:
        r.enable_step_count(False)
    print(what, "pixels", st["pixels"], "perturb_steps", st["perturb_steps"], "differing", int((frames[0] != frames[1]).sum()))
    assert np.array_equal(frames[0], frames[1]), what
    assert st["pixels"] == W * H, (what, st)
    if takes_steps:
        assert st["perturb_steps"] != 0, (what, st)
    return frames[1]


def _refused(r, setup, render, what):
    """A counting launch whose kernel has no counters: fs_read_step_count says so."""
    assert r.InitializeMemory(W, H, 1, None, 0, 0, 0, False) == 0
    assert setup() == 0
    try:
        r.enable_step_count(True)
        assert r.ClearMemory() == 0
        assert render() == 0
        assert r.SyncComputeStream() == 0
        out = (C.c_uint64 * 8)()
        assert r._lib.fs_read_step_count(r._h, out) == FS_ERR_UNSUPPORTED, what
    finally:
        r.enable_step_count(False)


@pytest.mark.parametrize("kind", ["f32", "f64", "2x32"])
def test_plain_lav2(renderer, native_libs, kind):
    from test_plain_oracle import shallow_view
    r = renderer
    vs = shallow_view("1e-12", W=W, H=H)
    pin = inputs.PlainInputs(vs, kind)
    for mode, _ in MODES:
        _counted(r, lambda: r.InitializePerturbPlain(0, pin), lambda: r.RenderPerturbLAv2Plain(pin, vs.num_iterations, Mode=mode),
                 vs.num_iterations, mode != LAV2_LAO, (kind, mode))


@pytest.mark.parametrize("mode", [LAV2_FULL, LAV2_PO, LAV2_LAO])
def test_hdr2x32_lav2(renderer, v5, mode):
    """(PO is the long case: every pixel of view 5 walks to its count step by step in HDRFloat<CudaDblflt>, 2.4e8 steps a frame.)"""
    r = renderer
    v = v5["v"]
    o, la = v5[True][0], inputs.LATable(v5[True][0], use_small_exponents=True)
    o2, la2 = inputs.Orbit2x32(o), inputs.LATable2x32(la)
    tr = [(float(c["head"]), float(c["tail"]), int(c["e"])) for c in v.coords_perturb_2x32(o2)]
    n = v.num_iterations
    _counted(r, lambda: r.InitializePerturb(0, o2, 0, None, la2),
             lambda: r.RenderPerturbLAv2(None, None, None, *tr, n, T=T_HDR2X32, Mode=mode), n, mode != LAV2_LAO, mode)


def test_direct(renderer, native_libs):
    r = renderer
    v0 = inputs.View.builtin(0, W, H)
    n = v0.num_iterations
    dx, dy, minx, maxy = v0.coords_direct_f64()
    _counted(r, lambda: 0, lambda: r.Render(None, minx, maxy, dx, dy, n, T=T_F64), n, True, "f64")
    for is64 in (False, True):
        dxh, dyh, mxh, myh = _pairs(v0.coords_direct_hdr(is64))
        _counted(r, lambda: 0, lambda: r.Render(None, mxh, myh, dxh, dyh, n, T=T_HDR64 if is64 else T_HDR32), n, True,
                 "hdr64" if is64 else "hdr32")
    for kind, ip, T in (("1x32", 1, T_F32), ("1x32", 8, T_F32), ("2x32", 4, T_2X32), ("2x64", 1, T_2X64), ("4x32", 1, T_4X32),
                        ("4x64", 1, T_4X64)):
        _counted(r, lambda: 0, lambda: r.RenderLowPrecision(None, v0.coords_direct_lp(kind), n, ip, T=T), n, True, (kind, ip))


@pytest.mark.parametrize("table", [True, False])
def test_plain_double_bla(renderer, v5, table):
    r = renderer
    v = v5["v"]
    of = inputs.OrbitF64(v)
    cof = of.coords()
    lib = r._lib

    def upload():
        assert lib.fs_upload_orbit(r._h, 0, T_F64, 4, of.data_ptr, of.count, of.count, of.period) == 0
        if table:
            return lib.fs_upload_bla(r._h, T_F64, of.level_ptrs, of.level_sizes, of.num_levels, of.lm2)
        return lib.fs_upload_bla(r._h, T_F64, None, None, 0, 0)
    _counted(r, upload, lambda: lib.fs_render_bla(r._h, T_F64, cof.ctypes.data, v.num_iterations), v.num_iterations, True, table)


@pytest.mark.parametrize("is64", [False, True])
@pytest.mark.parametrize("resident", [False, True])
def test_literal_lav2(renderer, v5, is64, resident):
    """set_kernel_variant(1), and the same kernel walking a waypoint-resident orbit (fs_set_compressed_orbit_mode 1)."""
    r = renderer
    v = v5["v"]
    ob, la = v5[is64][2:] if resident else v5[is64][:2]
    co = _pairs(v.coords_perturb(ob))
    n = v.num_iterations
    T = T_HDR64 if is64 else T_HDR32
    try:
        assert r.set_kernel_variant(1) == 0
        assert r.set_compressed_orbit_mode(resident) == 0
        frames = {}
        for mode, parity in MODES:
            frames[mode] = _counted(r, lambda: r.InitializePerturb(0, ob, 0, None, la),
                                    lambda: r.RenderPerturbLAv2(None, None, None, *co, n, T=T, Mode=mode, parity=parity), n,
                                    mode != LAV2_LAO, (is64, resident, mode))
        assert int(frames[LAV2_FULL].max()) > 0
    finally:
        r.set_compressed_orbit_mode(False)
        r.set_kernel_variant(0)


def test_no_counters_is_refused_not_read_as_zeros(renderer, v5):
    from test_plain_oracle import shallow_view
    r = renderer
    v = v5["v"]
    n = v.num_iterations
    try:
        # 64-bit counters
        ob, la = v5[False][:2]
        co = _pairs(v.coords_perturb(ob))
        assert r.set_kernel_variant(0, wide_counters=True) == 0
        _refused(r, lambda: r.InitializePerturb(0, ob, 0, None, la),
                 lambda: r.RenderPerturbLAv2(None, None, None, *co, n, T=T_HDR32, Mode=LAV2_FULL, parity=PARITY_CPU), "wide")
        assert r.set_kernel_variant(0) == 0
        # a plain and the 2x32 kernel on a waypoint-resident orbit
        assert r.set_compressed_orbit_mode(True) == 0
        vs = shallow_view("1e-12", W=W, H=H)
        pin = inputs.PlainInputs(vs, "f64", compression_exp=20)
        _refused(r, lambda: r.InitializePerturbPlain(0, pin), lambda: r.RenderPerturbLAv2Plain(pin, vs.num_iterations), "plain")
        o = v5[True][2]
        o2, la2 = inputs.Orbit2x32(o), inputs.LATable2x32(inputs.LATable(o, use_small_exponents=True))
        tr = [(float(c["head"]), float(c["tail"]), int(c["e"])) for c in v.coords_perturb_2x32(o2)]
        _refused(r, lambda: r.InitializePerturb(0, o2, 0, None, la2),
                 lambda: r.RenderPerturbLAv2(None, None, None, *tr, n, T=T_HDR2X32, Mode=LAV2_FULL), "2x32")
    finally:
        r.set_compressed_orbit_mode(False)
        r.set_kernel_variant(0)
