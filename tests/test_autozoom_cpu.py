"""CPU-only: the sequential autozoom checker (tests/autozoom/autozoom_ref.cpp) against its committed records
(tests/golden/autozoom_vectors.json), against an independent numpy statement of Max and FilamentTip on CPU-oracle frames and
synthetic ones, and fsh_view_autozoom_next against exact rational arithmetic on the views' bounding boxes."""
import json
import math
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

import _autozoom
from fractalshark_amd import _capi, autozoom, inputs


@pytest.fixture(scope="module")
def frames(native_libs):
    return _autozoom.frames()


@pytest.fixture(scope="module")
def golden():
    with open(_autozoom.GOLDEN) as f:
        return json.load(f)


def test_record_layout():
    import ctypes as C
    assert C.sizeof(_capi.AutozoomResult) == 200
    assert _capi.AutozoomResult.target_x.offset == 8 and _capi.AutozoomResult.high_hist.offset == 80
    assert _capi.AutozoomResult.score.offset == 168 and _capi.AutozoomResult.sum_sq_y.offset == 192


def test_checker_reproduces_the_fixture_for_both_iter_types(frames, golden):
    assert sorted(golden) == sorted(frames)
    for name, (frame, w, h, aa, n) in frames.items():
        g = golden[name]
        assert (g["width"], g["height"], g["antialiasing"], g["n_iterations"]) == (w, h, aa, n)
        for hname, heur in _autozoom.HEURISTICS.items():
            for dtype in (np.uint32, np.uint64):
                assert _autozoom.as_dict(_autozoom.ref_pick(frame.astype(dtype), w, h, heur, n, aa)) == g[hname], (name, hname)


# ---- an independent statement of Max and FilamentTip: whole-array numpy, no loop over pixels
def numpy_max(valid):
    top = int(valid.max())
    ys, xs = np.nonzero(valid == top)  # row-major order: the first entry is the first in raster order
    return (int(xs[0]), int(ys[0])), len(xs)


def numpy_tip(valid, n_iterations):
    h, w = valid.shape
    v = valid.astype(np.int64)
    avg = float(int(v.sum())) / float(w * h)
    threshold = int(avg + 1)
    m, r = 18, 12
    inner = v[m:h - m, m:w - m]
    cand = inner >= threshold
    ring = [(0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1)]
    high = np.stack([v[m + dy * r:h - m + dy * r, m + dx * r:w - m + dx * r] >= np.maximum(inner - 1, 0) for dx, dy in ring])
    count = high.sum(axis=0)
    # the longest run round the ring: k consecutive directions all high, for the largest such k (k <= 3 is all that matters)
    longest = np.zeros_like(count)
    for k in range(1, 9):
        has = np.zeros(count.shape, bool)
        for s in range(8):
            has |= np.all(high[[(s + i) % 8 for i in range(k)]], axis=0)
        longest[has] = k
    accepted = cand & (count <= 3) & ((count == 0) | (longest >= count))
    ys, xs = np.nonzero(accepted)
    cur = inner[ys, xs].astype(np.float64)
    best, best_xy = -1.0, None
    far = math.sqrt(float(w * w + h * h)) / 2.0
    for x, y, c, k in zip(xs + m, ys + m, cur, count[ys, xs]):  # (accepted candidates only; raster order)
        raw = math.log(1.0 + (c - avg)) / math.log(1.0 + (float(n_iterations) - avg)) if float(n_iterations) - avg > 0 else 0.5
        dist = math.sqrt(float(x - w // 2) ** 2 + float(y - h // 2) ** 2) / far
        score = (1.0 - float(k) / 4.0) * (1.0 - raw) * (0.3 + 0.7 * dist)
        if score > best:
            best, best_xy = score, (int(x), int(y))
    return best_xy, best, int(cand.sum()), int(accepted.sum())


def _tip_fields(res):
    return (int(res.target_x), int(res.target_y)), res.score, int(res.candidates), int(res.accepted)


def test_view0_max_and_tip_known_values(frames):
    frame, w, h, aa, n = frames["view0_384x216"]
    valid = frame[:h, :w]
    mx = _autozoom.ref_pick(frame, w, h, autozoom.MAX, n)
    assert numpy_max(valid) == ((186, 60), 4430)
    assert ((int(mx.target_x), int(mx.target_y)), int(mx.num_at_limit)) == ((186, 60), 4430)
    assert mx.status == autozoom.MOVE_THEN_STOP and mx.num_at_max == 4430
    tip = _autozoom.ref_pick(frame, w, h, autozoom.FILAMENT_TIP, n)
    assert _tip_fields(tip) == ((180, 64), 0.15717920107248098, 4456, 770)
    assert numpy_tip(valid, n) == _tip_fields(tip)
    assert tip.status == autozoom.MOVE


def test_view0_tip_winner_ties_with_its_mirror_image(frames):
    """View 0 is symmetric about the real axis, which is row H / 2 of the frame (row k mirrors row H - k; row 0 has no partner):
    the winner's mirror image scores the same to the bit, and the raster order -- the upper one first, strict `>` -- decides."""
    frame, w, h, aa, n = frames["view0_384x216"]
    tip = _autozoom.ref_pick(frame, w, h, autozoom.FILAMENT_TIP, n)
    # the same frame with the winner knocked out: its mirror image takes over with the SAME score
    knocked = frame.copy()
    knocked[64, 180] = 0
    second = _autozoom.ref_pick(knocked, w, h, autozoom.FILAMENT_TIP, n)
    assert (int(second.target_x), int(second.target_y)) == (180, h - 64)
    assert abs(second.score - tip.score) < 1e-4  # (not equal: removing a pixel moved the frame's average a little)


def test_view5_max_and_tip_known_values(frames):
    frame, w, h, aa, n = frames["view5_192x108"]
    valid = frame[:h, :w]
    mx = _autozoom.ref_pick(frame, w, h, autozoom.MAX, n)
    assert numpy_max(valid) == ((83, 56), 44)
    assert ((int(mx.target_x), int(mx.target_y)), int(mx.num_at_limit)) == ((83, 56), 44)
    tip = _autozoom.ref_pick(frame, w, h, autozoom.FILAMENT_TIP, n)
    assert _tip_fields(tip)[0] == (78, 22) and _tip_fields(tip)[2:] == (1897, 1754)
    assert numpy_tip(valid, n) == _tip_fields(tip)


def test_lattice_ties(frames):
    frame, w, h, aa, n = frames["lattice_144x256"]
    tip = _autozoom.ref_pick(frame, w, h, autozoom.FILAMENT_TIP, n)
    assert _tip_fields(tip) == ((20, 20), 0.0, 968, 968)
    assert numpy_tip(frame[:h, :w], n) == _tip_fields(tip)
    assert tip.status == autozoom.MOVE and list(tip.high_hist) == [968] + [0] * 8


def test_constant_frame(frames):
    frame, w, h, aa, n = frames["constant_96x80"]
    assert _autozoom.ref_pick(frame, w, h, autozoom.MAX, n).status == autozoom.FLAT
    assert _autozoom.ref_pick(frame, w, h, autozoom.DEFAULT, n).status == autozoom.FLAT
    tip = _autozoom.ref_pick(frame, w, h, autozoom.FILAMENT_TIP, n)
    assert tip.status == autozoom.NO_TARGET and tip.candidates == 0 and tip.score == -1.0
    zero = np.zeros_like(frame)
    assert _autozoom.ref_pick(zero, w, h, autozoom.FILAMENT_TIP, n).status == autozoom.NO_TARGET
    assert _autozoom.ref_pick(zero, w, h, autozoom.DEFAULT, n).status == autozoom.FLAT


def test_mirror_frame_and_last_row(frames):
    frame, w, h, aa, n = frames["mirror_128x96"]
    tip = _autozoom.ref_pick(frame, w, h, autozoom.FILAMENT_TIP, n)
    assert _tip_fields(tip)[0] == (30, 40) and tip.accepted == 4
    assert numpy_tip(frame[:h, :w], n) == _tip_fields(tip)
    frame, w, h, aa, n = frames["last_row_tip_100x90"]
    tip = _autozoom.ref_pick(frame, w, h, autozoom.FILAMENT_TIP, n)
    assert _tip_fields(tip)[0] == (w - 19, h - 19) and tip.accepted == 1


def test_default_numpy_statement(frames):
    """Default against a float statement in numpy: the integers exactly, the target to the bound two orders of summation may
    differ by (4 n 2^-53 relative: every term is non-negative, so each sum is within gamma_(n-1) of the true one in either
    order, and a quotient of two such sums doubles it)."""
    for name in ("view0_384x216", "view0_192x108_aa2", "view5_192x108", "mirror_128x96"):
        frame, w, h, aa, n = frames[name]
        sw, sh = w // aa, h // aa
        x0, x1, y0, y1 = sw // 8 * aa, (sw - sw // 8) * aa, sh // 8 * aa, (sh - sh // 8) * aa
        rect = frame[y0:y1, x0:x1].astype(np.float64)
        res = _autozoom.ref_pick(frame, w, h, autozoom.DEFAULT, n, aa)
        top, total = int(rect.max()), int(frame[y0:y1, x0:x1].astype(np.uint64).sum())
        avg = float(total) / float(rect.size)
        assert (res.max_iter, res.sum_iters, res.avg, res.num_at_limit) == (top, total, avg, int((rect == top).sum()))
        hw, hh = (x1 - x0) / 2.0, (y1 - y0) / 2.0
        ex = np.abs(hw - np.abs(hw - np.arange(x1 - x0, dtype=np.float64)))[None, :]
        ey = np.abs(hh - np.abs(hh - np.arange(y1 - y0, dtype=np.float64)))[:, None]
        weight = rect / float(n)
        weight = np.where(rect == top, weight * weight, weight)
        sq = np.where(rect >= avg, weight * (np.sqrt(ex * ex + ey * ey) / math.sqrt(hw * hw + hh * hh)), 0.0)
        assert res.num_at_max == int(((rect >= avg) & (rect >= n)).sum())
        tx = float((sq * np.arange(x0, x1)[None, :]).sum() / sq.sum())
        ty = float((sq * np.arange(y0, y1)[:, None]).sum() / sq.sum())
        bound = 4 * rect.size * 2.0 ** -53
        assert abs(res.target_x - tx) <= bound * tx and abs(res.target_y - ty) <= bound * ty, name


# ---- the next view
def _box(view):
    # (through Decimal: exact, and deep views print thousands of digits, more than int() takes from a string by default)
    return [Fraction(Decimal(s)) for s in view.bbox()]


@pytest.mark.parametrize("view_no,width,height,aa", [(0, 384, 216, 1), (5, 192, 108, 1), (5, 192, 108, 2), (14, 160, 90, 1)])
@pytest.mark.parametrize("divisor,x,y", [(32, 186.0, 60.0), (8, 20.0, 71.0), (3, 85.7789452023929, 59.347942738050754), (8, 0.0, 0.0)])
def test_next_view_against_exact_rationals(native_libs, view_no, width, height, aa, divisor, x, y):
    v = inputs.View.builtin(view_no, width, height, antialiasing=aa)
    min_x, min_y, max_x, max_y = _box(v)
    w_aa, h_aa = width * aa, height * aa
    gx = min_x + Fraction(x) * (max_x - min_x) / w_aa
    gy = max_y - Fraction(y) * (max_y - min_y) / h_aa
    want = [gx - (max_x - min_x) / divisor, gy - (max_y - min_y) / divisor, gx + (max_x - min_x) / divisor,
            gy + (max_y - min_y) / divisor]
    nv = v.autozoom_next(x, y, divisor)
    got = _box(nv)
    pitch = (want[2] - want[0]) / w_aa  # of the new view
    for g, t in zip(got, want):
        assert abs(g - t) <= pitch / 2 ** 64
    # the new view is 2 / divisor of the old one, both ways
    for a, b in (((got[2] - got[0]), (max_x - min_x)), ((got[3] - got[1]), (max_y - min_y))):
        assert abs(a / b - Fraction(2, divisor)) <= Fraction(1, 2 ** 64)
    assert (nv.width, nv.height, nv.num_iterations, nv.antialiasing) == (width, height, v.num_iterations, aa)
    # ... and carries the precision a view made from its box would be given
    assert nv.precision_bits == inputs.View(*nv.bbox(), width, height).precision_bits


def test_next_view_refuses_bad_arguments(native_libs):
    v = inputs.View.builtin(0, 64, 36)
    for args in ((float("nan"), 0.0, 8), (0.0, float("inf"), 8), (1.0, 1.0, 0)):
        with pytest.raises(ValueError):
            v.autozoom_next(*args)


def test_next_view_of_a_pick(frames):
    frame, w, h, aa, n = frames["view0_384x216"]
    v = inputs.View.builtin(0, w, h)
    mx = _autozoom.ref_pick(frame, w, h, autozoom.MAX, n)
    assert autozoom.next_view(v, mx).bbox() == v.autozoom_next(186.0, 60.0, 32).bbox()
    flat = _autozoom.ref_pick(np.zeros_like(frame), w, h, autozoom.MAX, n)
    with pytest.raises(ValueError):
        autozoom.next_view(v, flat)
