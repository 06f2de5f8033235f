"""Shared by the autozoom tests: the sequential checker (tests/autozoom/autozoom_ref.cpp) over host frames, the frames the
tests use, and records as plain dicts."""
import ctypes as C
import os
import subprocess

import numpy as np

import _oracle
from fractalshark_amd import _capi, autozoom, inputs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
AZ_DIR = os.path.join(HERE, "autozoom")
GOLDEN = os.path.join(HERE, "golden", "autozoom_vectors.json")
HEURISTICS = {"default": autozoom.DEFAULT, "max": autozoom.MAX, "tip": autozoom.FILAMENT_TIP}
INT_FIELDS = ("status", "heuristic", "max_iter", "num_at_limit", "num_at_max", "sum_iters", "candidates", "accepted", "run_reject")
FLOAT_FIELDS = ("target_x", "target_y", "avg", "score", "sum_sq", "sum_sq_x", "sum_sq_y")

_lib = None


def checker_lib():
    """g++ build of tests/autozoom/autozoom_ref.cpp."""
    global _lib
    if _lib is None:
        lib = os.path.join(AZ_DIR, "libautozoom_ref.so")
        srcs = [os.path.join(AZ_DIR, "autozoom_ref.cpp"), os.path.join(ROOT, "include", "fs_layout.h")]
        if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
            subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", lib, srcs[0]], check=True)
        _lib = C.CDLL(lib)
        _lib.azr_pick.restype = C.c_int
        _lib.azr_pick.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                  C.POINTER(_capi.AutozoomResult)]
    return _lib


def ref_pick(frame, w, h, heuristic, n_iterations, aa=1):
    """The checker's record for the valid w x h part of `frame` (2-D uint32 / uint64, rows of any pitch >= w)."""
    frame = np.ascontiguousarray(frame)
    assert frame.dtype in (np.uint32, np.uint64) and frame.shape[0] >= h and frame.shape[1] >= w
    res = _capi.AutozoomResult()
    assert checker_lib().azr_pick(int(heuristic), frame.ctypes.data, 1 if frame.dtype == np.uint64 else 0, frame.shape[1], w, h,
                                  aa, int(n_iterations), C.byref(res)) == 0
    return res


def as_dict(res):
    """Every field of a record but `rescored` (what the library's host side scored: not a quantity of the checker), floats as
    their exact hexadecimal text."""
    d = {k: int(getattr(res, k)) for k in INT_FIELDS}
    d.update({k: float(getattr(res, k)).hex() for k in FLOAT_FIELDS})
    d["high_hist"] = [int(v) for v in res.high_hist]
    return d


def padded(valid, dtype=np.uint32):
    """A frame in the layout of the iteration buffer: rows of a multiple of 16 elements, a multiple of 8 rows."""
    h, w = valid.shape
    out = np.zeros(((h + 7) // 8 * 8, (w + 15) // 16 * 16), dtype)
    out[:h, :w] = valid
    return out


# ---- synthetic frames (valid part, uint32)
LATTICE_N = 1000


def lattice(w=144, h=256, n=LATTICE_N):
    """Zero except n where a fifth row meets a fifth column: every lattice pixel inside the margin is an isolated peak at the
    iteration limit and scores exactly 0 -- hundreds of exact ties."""
    f = np.zeros((h, w), np.uint32)
    f[::5, ::5] = n
    return f


def constant(w=96, h=80, value=7):
    return np.full((h, w), value, np.uint32)


def mirror(w=128, h=96):
    """Left-right mirror-symmetric about the frame's centre column W / 2: isolated peaks at x and W - x tie exactly (the score
    depends on |x - W / 2| only), so the raster tie-break decides."""
    f = np.full((h, w), 10, np.uint32)
    for (x, y, v) in ((30, 40, 50), (w - 30, 40, 50), (44, 60, 50), (w - 44, 60, 50)):
        f[y, x] = v
    return f


def last_row_tip(w=100, h=90):
    """One isolated peak in the last row the margin admits."""
    f = np.full((h, w), 3, np.uint32)
    f[h - 19, w - 19] = 40
    return f


def oracle_view0(width=384, height=216, aa=1):
    v = inputs.View.builtin(0, width, height, antialiasing=aa)
    return v, _oracle.direct_f64(v, aa=aa, n_iterations=8192), 8192


def oracle_view5(width=192, height=108):
    v = inputs.View.builtin(5, width, height, antialiasing=1)
    ob = inputs.Orbit(v)
    la = inputs.LATable(ob)
    return v, _oracle.lav2_hdr32(v, ob, la, stage_test=0), v.num_iterations


def frames():
    """name -> (frame in buffer layout, w, h, antialiasing, n_iterations) of every frame the fixture records."""
    out = {}
    _, f0, n0 = oracle_view0()
    out["view0_384x216"] = (f0, 384, 216, 1, n0)
    _, f0a, _ = oracle_view0(192, 108, 2)
    out["view0_192x108_aa2"] = (f0a, 384, 216, 2, n0)
    _, f5, n5 = oracle_view5()
    out["view5_192x108"] = (f5, 192, 108, 1, n5)
    for name, valid, n in (("lattice_144x256", lattice(), LATTICE_N), ("constant_96x80", constant(), 100),
                           ("mirror_128x96", mirror(), 100), ("last_row_tip_100x90", last_row_tip(), 100)):
        out[name] = (padded(valid), valid.shape[1], valid.shape[0], 1, n)
    return out


# ---- the GPU side (tests/test_gpu_autozoom.py and its child process tests/autozoom/torch_frames.py)
def gpu_pick(r, heuristic, n, device_iters=None):
    err, res = r.AutozoomPick(heuristic, n, device_iters)
    assert err == 0, r.ConvertErrorToString(err)
    return res


def _bytes_without_rescored(res):
    c = type(res).from_buffer_copy(res)
    c.rescored = 0
    return bytes(c)


def check_against_checker(r, frame, w, h, aa, n, device_iters=None):
    """Every heuristic on the renderer's current frame (or device_iters) against the checker on its host copy `frame`."""
    got = {}
    for name in ("max", "tip"):
        heur = HEURISTICS[name]
        if name == "tip" and (w <= 36 or h <= 36):
            continue
        ref = ref_pick(frame, w, h, heur, n, aa)
        res = gpu_pick(r, heur, n, device_iters)
        print(name, as_dict(res), "rescored", res.rescored)
        assert as_dict(res) == as_dict(ref), name
        assert _bytes_without_rescored(res) == _bytes_without_rescored(ref), name
        if name == "tip":
            assert (res.rescored >= 1 if res.accepted else res.rescored == 0) and res.rescored <= res.accepted
        got[name] = res
    ref = ref_pick(frame, w, h, autozoom.DEFAULT, n, aa)
    res, again = gpu_pick(r, autozoom.DEFAULT, n, device_iters), gpu_pick(r, autozoom.DEFAULT, n, device_iters)
    print("default", as_dict(res), "checker", ref.target_x, ref.target_y)
    assert bytes(res) == bytes(again)  # a fixed tree: bitwise the same from run to run
    for k in INT_FIELDS:
        assert getattr(res, k) == getattr(ref, k), k
    assert res.avg == ref.avg and list(res.high_hist) == list(ref.high_hist) == [0] * 9
    # all terms are non-negative: each sum, in either order, is within gamma_(n-1) of the true sum, a quotient of two such sums
    # doubles the bound -- 4 n 2^-53 relative, n = pixels of the rectangle.  Derived, not measured.
    sw, sh = w // aa, h // aa
    n_rect = ((sw - sw // 8) * aa - sw // 8 * aa) * ((sh - sh // 8) * aa - sh // 8 * aa)
    bound = 4 * n_rect * 2.0 ** -53
    for k in ("target_x", "target_y"):
        a, b = getattr(res, k), getattr(ref, k)
        print(k, "relative difference", abs(a - b) / abs(b) if b else abs(a - b), "bound", bound)
        assert abs(a - b) <= bound * abs(b), k
    got["default"] = res
    return got


def read_frame(r, n):
    out = r.new_iter_buffer()
    assert r.RenderCurrent(n, out) == 0
    assert r.SyncComputeStream() == 0
    return out
