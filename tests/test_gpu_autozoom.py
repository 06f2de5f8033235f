"""fs_autozoom_pick on the GPU against the sequential checker (tests/autozoom/autozoom_ref.cpp) on the SAME frame: Max and
FilamentTip byte for byte (every field but `rescored`, which counts the library's own host work), Default in its integers, its
determinism and the derived bound of its two quotients.  Frames rendered on the GPU (and equal to the CPU oracle's), both
IterTypes, antialiasing 1 and 2, and synthetic frames in torch device tensors; error codes; frame state; the zoom loop."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _autozoom
import _oracle
from fractalshark_amd import (GPURenderer, LAV2_FULL, PARITY_CPU, T_F64, T_HDR32, autozoom, inputs)
from fractalshark_amd.renderer import FS_ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu

FS_ERR_6 = 10005


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.close()


def _render_view0(r, v, n, iter_bytes=4):
    aa = v.antialiasing
    assert r.InitializeMemory(v.width * aa, v.height * aa, aa, None, 0, 0, 0, False, iter_bytes=iter_bytes) == 0
    dx, dy, minx, maxy = v.coords_direct_f64()
    assert r.Render(None, minx, maxy, dx, dy, n, T=T_F64) == 0


@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("cap_rows", [0, 2])
def test_view0_direct_frame(renderer, aa, cap_rows):
    r = renderer
    v, oracle_frame, n = _autozoom.oracle_view0(384 // aa, 216 // aa, aa)
    _render_view0(r, v, n)
    frame = _autozoom.read_frame(r, n)
    assert np.array_equal(frame, oracle_frame)
    assert r.SetAutozoomGatherCap(cap_rows) == 0
    try:
        got = _autozoom.check_against_checker(r, frame, 384, 216, aa, n)
    finally:
        assert r.SetAutozoomGatherCap(0) == 0
    assert (got["max"].target_x, got["max"].target_y, got["max"].num_at_limit) == (186, 60, 4430)
    assert (got["tip"].target_x, got["tip"].target_y, got["tip"].score) == (180, 64, 0.15717920107248098)
    assert (got["tip"].candidates, got["tip"].accepted) == (4456, 770)


@pytest.mark.parametrize("iter_bytes", [4, 8])
def test_view5_lav2_hdr32_cpu_parity_frame(renderer, iter_bytes):
    r = renderer
    v, oracle_frame, n = _autozoom.oracle_view5()
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    assert r.InitializeMemory(v.width, v.height, 1, None, 0, 0, 0, False, iter_bytes=iter_bytes) == 0
    assert r.InitializePerturb(0, ob, 0, None, inputs.LATableU64(la) if iter_bytes == 8 else la, iter_bytes=iter_bytes) == 0
    assert r.ClearMemory() == 0
    dx, dy, cx, cy = [(float(c["m"]), int(c["e"])) for c in v.coords_perturb(ob)]
    assert r.RenderPerturbLAv2(None, None, None, dx, dy, cx, cy, n, T=T_HDR32, Mode=LAV2_FULL, parity=PARITY_CPU) == 0
    frame = _autozoom.read_frame(r, n)
    assert frame.dtype == (np.uint64 if iter_bytes == 8 else np.uint32) and np.array_equal(frame, oracle_frame)
    got = _autozoom.check_against_checker(r, frame, v.width, v.height, 1, n)
    assert (got["max"].target_x, got["max"].target_y, got["max"].num_at_limit) == (83, 56, 44)
    assert (got["tip"].target_x, got["tip"].target_y, got["tip"].candidates, got["tip"].accepted) == (78, 22, 1897, 1754)
    assert r.InitializeMemory(v.width, v.height, 1, None, 0, 0, 0, False, iter_bytes=4) == 0


@pytest.fixture(scope="module")
def torch_child():
    """The synthetic frames live in torch device tensors, and torch has to bring the GPU up BEFORE libfsmi355.so touches it; in
    this process the library has long done so.  So those cases run in one fresh child process (tests/autozoom/torch_frames.py),
    which reports per case; the tests below look their case up."""
    script = os.path.join(_autozoom.AZ_DIR, "torch_frames.py")
    p = subprocess.run([sys.executable, script], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULTS ")][-1]
    return json.loads(line[len("RESULTS "):])


@pytest.mark.parametrize("dtype", ["uint32", "uint64"])
@pytest.mark.parametrize("cap_rows", [0, 2])
@pytest.mark.parametrize("name", ["constant", "last_row_tip", "lattice", "mirror"])
def test_synthetic_frames_in_a_torch_tensor(torch_child, name, cap_rows, dtype):
    """Lattice, constant, mirror-symmetric and last-eligible-row frames through SetExternalIterBuffer, both IterTypes, with the
    default gather buffer and with two rows of it (the lattice's 968 exact ties then go through the band path)."""
    assert torch_child["%s-%d-%s" % (name, cap_rows, dtype)] == "ok"


def test_device_iters_argument_leaves_the_current_buffer_alone(torch_child):
    assert torch_child["device_iters"] == "ok"


def test_error_codes(renderer):
    fresh = GPURenderer(0)
    try:
        assert fresh.AutozoomPick(autozoom.MAX, 100)[0] == FS_ERR_6
    finally:
        fresh.close()
    r = renderer
    assert r.InitializeMemory(64, 48, 1, None, 0, 0, 0, False) == 0
    assert r.AutozoomPick(3, 100)[0] == FS_ERR_UNSUPPORTED and r.AutozoomPick(-1, 100)[0] == FS_ERR_UNSUPPORTED
    assert r.AutozoomPick(autozoom.MAX, 100)[0] == 0
    assert r.SetRowBands(0, 8, 16) == 0
    try:
        for heur in (autozoom.DEFAULT, autozoom.MAX, autozoom.FILAMENT_TIP):
            assert r.AutozoomPick(heur, 100)[0] == FS_ERR_UNSUPPORTED
    finally:
        assert r.SetRowBands(0, 0, 0) == 0
    # FilamentTip needs a pixel inside its 18-pixel margin
    for w, h in ((36, 64), (64, 36), (32, 32)):
        assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False) == 0
        assert r.AutozoomPick(autozoom.FILAMENT_TIP, 100)[0] == FS_ERR_UNSUPPORTED
        assert r.AutozoomPick(autozoom.MAX, 100)[0] == 0 and r.AutozoomPick(autozoom.DEFAULT, 100)[0] == 0
    assert r.InitializeMemory(37, 37, 1, None, 0, 0, 0, False) == 0
    assert r.AutozoomPick(autozoom.FILAMENT_TIP, 100)[0] == 0


def test_frame_state_is_left_as_it_was(renderer):
    r = renderer
    v, _, n = _autozoom.oracle_view0(192, 108, 1)
    _render_view0(r, v, n)
    before = _autozoom.read_frame(r, n)
    ms, history = r.last_kernel_ms(), r.kernel_ms_history(1)
    assert ms > 0
    for heur in (autozoom.DEFAULT, autozoom.MAX, autozoom.FILAMENT_TIP):
        _autozoom.gpu_pick(r, heur, n)
    assert r.last_kernel_ms() == ms and r.kernel_ms_history(1) == history
    assert _autozoom.read_frame(r, n).tobytes() == before.tobytes()


@pytest.mark.parametrize("heuristic", [autozoom.MAX, autozoom.FILAMENT_TIP])
def test_zoom_loop_matches_the_checker_driven_loop(renderer, heuristic):
    """autozoom.zoom for four steps from View 0 (direct render) against the same loop with CPU-oracle frames and the checker:
    the same bounding boxes, digit for digit, and the same stop."""
    r = renderer
    w, h, steps = 384, 216, 4
    v0 = inputs.View.builtin(0, w, h, antialiasing=1)

    def render(rr, view):
        _render_view0(rr, view, view.num_iterations)

    got = [(p.status, nv.bbox() if nv is not None else None) for _, p, nv in autozoom.zoom(r, v0, heuristic, render, steps)]
    want, view = [], v0
    for _ in range(steps):
        frame = _oracle.direct_f64(view)
        p = _autozoom.ref_pick(frame, w, h, heuristic, view.num_iterations)
        if p.status in (autozoom.FLAT, autozoom.NO_TARGET):
            want.append((p.status, None))
            break
        nv = autozoom.next_view(view, p)
        want.append((p.status, nv.bbox()))
        if p.status == autozoom.MOVE_THEN_STOP:
            break
        view = nv
    print(heuristic, [s for s, _ in got])
    assert got == want and len(got) >= 1
    if heuristic == autozoom.FILAMENT_TIP:
        assert len(got) == steps and all(s == autozoom.MOVE for s, _ in got)
