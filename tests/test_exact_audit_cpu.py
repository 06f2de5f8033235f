"""CPU-only: the rule of fs_exact_audit (csrc/exact_audit_math.hpp) built for the host with g++ (tests/exact/exact_audit_host.cpp,
the kernel's one wave as a loop over 64 lanes) against a numpy restatement (tests/_audit.py): 0 and 8 levels, all equal, all
differing, capped samples, more than 16 offenders, uint32 and uint64 frames, sample counts around the 64-lane chunk.  Then
exact.lattice against the fixture's lattice and finest_clean_level on hand-made reports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _audit
import _truth
from fractalshark_amd import _capi, exact

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "exact", "exact_audit_host.cpp")
HDRS = [os.path.join(os.path.dirname(HERE), "fractalshark_amd", "csrc", "exact_audit_math.hpp"),
        os.path.join(os.path.dirname(HERE), "include", "fs_layout.h")]
SO = os.path.join(HERE, "exact", "libexact_audit_host.so")
CAP = 20000


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or max(os.path.getmtime(p) for p in [SRC] + HDRS) > os.path.getmtime(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC], check=True)
    return C.CDLL(SO)


def _run(lib, frame, xs, ys, exact_counts, stable, cap=CAP, wrong_run=3):
    """The host walk over a frame (2-D array, its row length the pitch) and run counts made from (exact, stable): the four runs of
    a level equal the exact count where the sample is stable there, and run `wrong_run` of the four is off by one where not."""
    n, k = len(xs), stable.shape[1]
    counts = np.tile(np.asarray(exact_counts, np.uint64), (1 + 4 * k, 1))
    for j in range(k):
        counts[1 + 4 * j + (wrong_run + j) % 4, ~stable[:, j]] += 1
    counts = np.ascontiguousarray(counts)
    xs, ys = np.ascontiguousarray(xs, np.uint32), np.ascontiguousarray(ys, np.uint32)
    res = _capi.AuditResult()
    ex, fr, st = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    frame = np.ascontiguousarray(frame)
    lib.exa_audit(C.c_void_p(frame.ctypes.data), C.c_int(frame.itemsize == 8), C.c_uint32(frame.shape[1]), C.c_void_p(xs.ctypes.data),
                  C.c_void_p(ys.ctypes.data), C.c_void_p(counts.ctypes.data), C.c_uint32(n), C.c_uint32(k), C.c_uint64(cap),
                  C.byref(res), C.c_void_p(ex.ctypes.data), C.c_void_p(fr.ctypes.data), C.c_void_p(st.ctypes.data))
    return res, ex, fr, st


def _case(rng, n, k, dtype, differ_share, capped_share, w=37, h=23, pitch=48):
    """n samples (pixels may repeat) of a w x h frame with `pitch` elements per row."""
    xs, ys = rng.integers(0, w, n), rng.integers(0, h, n)
    frame = rng.integers(0, CAP, (h, pitch)).astype(dtype)
    exact_counts = frame[ys, xs].astype(np.int64)
    # (a pixel sampled twice must get one exact value: decide per pixel, not per sample)
    per_pixel = rng.random((h, w))
    capped = per_pixel[ys, xs] < capped_share
    exact_counts[capped] = CAP
    off = rng.integers(1, 1000, (h, w))[ys, xs] * np.where(rng.random((h, w))[ys, xs] < 0.5, -1, 1)
    differ = rng.random((h, w))[ys, xs] < differ_share
    exact_counts[differ & ~capped] = np.maximum(0, exact_counts + off)[differ & ~capped]
    stable = rng.random((n, k)) < 0.6
    return frame, xs, ys, exact_counts, stable


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("k", [0, 1, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 576])
def test_record_equals_numpy(lib, n, k, dtype):
    assert lib.exa_record_bytes() == C.sizeof(_capi.AuditResult) == 568
    rng = np.random.default_rng(1000 * n + 10 * k + np.dtype(dtype).itemsize)
    for differ_share, capped_share in ((0.3, 0.2), (0.0, 0.0), (1.0, 0.0), (0.02, 0.5)):
        frame, xs, ys, ex, stable = _case(rng, n, k, dtype, differ_share, capped_share)
        res, got_ex, got_fr, got_st = _run(lib, frame, xs, ys, ex, stable)
        fv = frame[ys, xs].astype(np.int64)
        want = _audit.expected(fv, ex, stable, CAP)
        _audit.same_record(res, want)
        assert np.array_equal(got_ex.astype(np.int64), ex) and np.array_equal(got_fr.astype(np.int64), fv)
        assert np.array_equal(got_st.astype(np.int64), want["stable_bits"])


def test_all_equal_all_differ_and_more_than_16_offenders(lib):
    rng = np.random.default_rng(5)
    n, k = 200, 8
    xs, ys = np.arange(n) % 20, np.arange(n) // 20
    frame = rng.integers(1, CAP, (10, 32)).astype(np.uint32)
    fv = frame[ys, xs].astype(np.int64)
    stable = rng.random((n, k)) < 0.5
    res, *_ = _run(lib, frame, xs, ys, fv, stable)                       # all equal
    assert (res.n_equal, res.n_differ, res.n_offenders) == (n, 0, 0) and not any(res.max_abs_diff) and not any(res.stable_differ)
    _audit.same_record(res, _audit.expected(fv, fv, stable, CAP))
    res, *_ = _run(lib, frame, xs, ys, fv + 7, stable)                   # all differ: 200 offenders, 16 recorded
    assert (res.n_equal, res.n_differ, res.n_offenders) == (0, n, 16)
    assert [o.sample for o in res.offenders] == list(range(16)) and list(res.max_abs_diff) == [7] * 8
    assert list(res.stable_differ) == list(res.stable)
    _audit.same_record(res, _audit.expected(fv, fv + 7, stable, CAP))
    ex = fv.copy()
    ex[[3, 70, 130, 199]] += 5                                          # offenders across chunk boundaries, in sample order
    res, *_ = _run(lib, frame, xs, ys, ex, stable)
    assert [o.sample for o in res.offenders[:res.n_offenders]] == [3, 70, 130, 199]
    _audit.same_record(res, _audit.expected(fv, ex, stable, CAP))


def test_capped_samples_and_values_beyond_32_bits(lib):
    cap = (1 << 40) + 5
    frame = np.array([[cap, cap - 1, 3, cap, 0, 0, 0, 0]], np.uint64)
    xs, ys = np.arange(4), np.zeros(4, np.int64)
    ex = np.array([cap, cap, 3, 1], np.int64)
    stable = np.array([[True, True], [True, False], [False, False], [False, True]])
    res, *_ = _run(lib, frame, xs, ys, ex, stable, cap=cap)
    assert (res.n_capped, res.n_differ, res.n_equal) == (2, 2, 2)
    assert list(res.stable[:2]) == [2, 2] and list(res.stable_capped[:2]) == [2, 1] and list(res.stable_differ[:2]) == [1, 1]
    assert list(res.max_abs_diff[:2]) == [1, cap - 1]
    _audit.same_record(res, _audit.expected(frame[0, :4].astype(np.int64), ex, stable, cap))


class _View:
    def __init__(self, w, h, aa=1):
        self.width, self.height, self.antialiasing = w // aa, h // aa, aa


@pytest.mark.parametrize("w,h,cols,rows", [(64, 36, 32, 18), (3840, 2160, 24, 12)])
@pytest.mark.parametrize("aa", [1, 2])
def test_lattice_is_the_fixtures(w, h, cols, rows, aa):
    xs, ys = exact.lattice(_View(w, h, aa), cols, rows)
    tx, ty = _truth.lattice(w, h, cols, rows)
    assert xs.dtype == ys.dtype == np.uint32 and np.array_equal(xs, tx) and np.array_equal(ys, ty)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (0, w - 1, 0, h - 1) and len(xs) == cols * rows


def test_the_fixture_cases_use_that_lattice():
    for name, cols, rows in (("shallow_1e-20", 32, 18), ("view5_3840x2160", 24, 12)):
        c = _truth.Case(name)
        xs, ys = exact.lattice(_View(c.w, c.h), cols, rows)
        assert np.array_equal(xs, c.xs) and np.array_equal(ys, c.ys)


def test_finest_clean_level_on_hand_made_reports():
    R = exact.AuditReport
    lv = (10, 15, 17, 20, 22, 25, 30, 35)
    # the HDRFloat<float> picture of the fixture's shallow_1e-20: clean to 2^-17, and 2^-10 holds no sample
    r = R(lv, 576, [0, 106, 209, 318, 388, 453, 520, 554], [0, 0, 0, 12, 55, 108, 174, 208])
    assert r.finest_clean_level() == 17
    assert r.finest_clean_level(min_samples=210) is None            # 209 stable samples are one short
    assert r.finest_clean_level(min_share=0.37) is None             # and 36.3 % of the samples
    assert r.finest_clean_level(min_samples=1, min_share=0.0) == 17
    # everything clean: the finest
    assert R(lv, 576, [0, 106, 209, 318, 388, 453, 520, 554], [0] * 8).finest_clean_level() == 35
    # a miss at a coarse level does not hide a clean finer one (each level is judged by itself), and order does not matter
    assert R((30, 17), 576, [520, 209], [0, 1]).finest_clean_level() == 30
    # the floors are those of the fixture: 100 samples and 20 %
    assert R((20,), 500, [100], [0]).finest_clean_level() == 20 and R((20,), 500, [99], [0]).finest_clean_level() is None
    assert R((20,), 501, [100], [0]).finest_clean_level() is None
    assert _truth.meets_floors(100, 500) and not _truth.meets_floors(99, 500) and not _truth.meets_floors(100, 501)
    assert (exact.MIN_STABLE_SAMPLES, exact.MIN_STABLE_SHARE) == (_truth.MIN_STABLE_SAMPLES, _truth.MIN_STABLE_SHARE)
    assert R((), 10, [], []).finest_clean_level() is None
