"""The exact renderer: fixed-point escape counts at any depth on the GPU, with no reference orbit and no rounding.

The render path of the reference's CpuHigh (CalcCpuHDR<IterType, HighPrecision, double>, Fractal.cpp:1200-1201, 2096-2206): every
sample is iterated by itself in high precision.  Here that is integer arithmetic on 32-bit limbs (csrc/exact_math.hpp,
csrc/kernels_exact.hip): x' = floor((x^2 - y^2) / 2^F) + cx, y' = floor(2xy / 2^F) + cy, escape when x^2 + y^2 > R 2^2F.  The frame
equals GMP integer iteration of that recurrence on every pixel, and is an ordinary frame in the renderer's iteration buffer:
min(E - 1, N) like every other path.  The axes come from the view's bounding-box strings read as exact rationals
(fsh_view_exact_axes).

audit() asks the library which sample pixels of a frame ANOTHER kernel rendered differ from those counts, and at which stability
levels the frame is clean (fs_exact_audit: the runs of all samples and ladder positions as one list on the device, the frame read
next to them, one small record back).

prove_interior=True on render, stable_mask and audit switches the cycle check on for the call (fs_set_exact_cycle_check; DESIGN.md
6.3 "Cycle check"): a sample whose state repeats exactly is proved never to escape and stops at once instead of running to the cap.
No count changes; frames with an interior at a shallow or middle depth get cheaper.  The wide path has no such check.

keep=True on render leaves the samples that reached the cap on the device (fs_set_exact_keep; DESIGN.md 6.3 "Continuation"), and
continue_render raises the frame's cap from there instead of starting over; render_progressive is the chain cap after cap.
"""
import numpy as np

GUARD_BITS = 64  # default frac_bits = the view's precision + this
MIN_LIMBS, MAX_LIMBS = 2, 24  # instantiated limb counts (csrc/exact_math.hpp)
MAX_FRAC_BITS = 32 * MAX_LIMBS - 10
MAX_WIDE_LIMBS = 704  # one wave per sample, 11 limbs per lane at the most (csrc/exact_wide_math.hpp)
MAX_WIDE_FRAC_BITS = 32 * MAX_WIDE_LIMBS - 10


def limbs_for(frac_bits):
    """The limb count a frac_bits needs: ceil((F + 10) / 32) (the bound is derived in csrc/exact_math.hpp), at least 2."""
    return max(MIN_LIMBS, (int(frac_bits) + 10 + 31) // 32)


def axes(view, frac_bits, level=None, limbs=None):
    """(cx, cy) = uint32[limbs, W], uint32[limbs, H]: c * 2^frac_bits per column / row of the antialiased frame, two's complement,
    limb-major.  With a ladder level, (cx3, cy3) = uint32[3, limbs, W], uint32[3, limbs, H]: the axes c, c + s, c - s with
    s = (maxX - minX) / 2^level."""
    limbs = limbs_for(frac_bits) if limbs is None else int(limbs)
    w, h = view.width * view.antialiasing, view.height * view.antialiasing
    n = 1 if level is None else 3
    cx, cy = np.zeros((n, limbs, w), np.uint32), np.zeros((n, limbs, h), np.uint32)
    if view._lib.fsh_view_exact_axes(view._h, w, h, int(frac_bits), -1 if level is None else int(level), limbs, cx.ctypes.data,
                                     cy.ctypes.data) != 0:
        raise ValueError("fsh_view_exact_axes: the view does not fit %d limbs at %d fractional bits" % (limbs, frac_bits))
    return (cx[0], cy[0]) if level is None else (cx, cy)


def _check(renderer, err, what):
    if err:
        raise RuntimeError("%s failed: %d (%s)" % (what, err, renderer.ConvertErrorToString(err)))


class _cycle_check:
    """The cycle check on for the duration of a call, off again behind it."""

    def __init__(self, renderer, on):
        self.renderer, self.on = renderer, bool(on)

    def __enter__(self):
        if self.on:
            _check(self.renderer, self.renderer.SetExactCycleCheck(True), "fs_set_exact_cycle_check")

    def __exit__(self, *exc):
        if self.on:
            self.renderer.SetExactCycleCheck(False)


def _proved(renderer, n=None):
    err, mask = renderer.ExactProved(n)
    _check(renderer, err, "fs_read_exact_proved")
    return mask.astype(bool)


class _keep:
    """Keeping on or off for the duration of a call, and behind it what the caller had set with SetExactKeep (off if never)."""

    def __init__(self, renderer, on):
        self.renderer, self.on = renderer, bool(on)

    def __enter__(self):
        self.before = bool(getattr(self.renderer, "_exact_keep", False))
        if self.on != self.before:
            _check(self.renderer, self.renderer.SetExactKeep(self.on), "fs_set_exact_keep")

    def __exit__(self, *exc):
        if self.on != self.before:
            self.renderer.SetExactKeep(self.before)


def render(renderer, view, bailout=4, frac_bits=None, iter_bytes=4, inclusive=False, prove_interior=False, keep=False,
           n_iterations=None):
    """The view's exact frame into the renderer's iteration buffer (InitializeMemory with the view's antialiased size and
    iter_bytes comes first), view.num_iterations the cap.  frac_bits defaults to view.precision_bits + 64.  Has the shape
    autozoom.zoom wants for its `render` argument.  Up to 24 limbs (758 bits) a lane holds a sample (fs_render_exact); beyond, a
    wave does (fs_render_exact_wide), up to 704 limbs.
    prove_interior: the cycle check is on for the call, and the result is bool[H, W], the samples it proved never to escape (they
    hold the cap, like those that ran to it).  On the wide path the check stays off and the result is None, as without it.
    keep: the samples that reach the cap stay on the device for continue_render (renderer.ExactKept() describes them); without it
    nothing is kept.  n_iterations: the cap, in place of view.num_iterations."""
    F = view.precision_bits + GUARD_BITS if frac_bits is None else int(frac_bits)
    L = limbs_for(F)
    cx, cy = axes(view, F, limbs=L)
    cap = view.num_iterations if n_iterations is None else int(n_iterations)
    with _keep(renderer, keep):
        if uses_wide(L):
            _check(renderer, renderer.RenderExactWide(iter_bytes, F, L, cx, cy, bailout, inclusive, cap), "fs_render_exact_wide")
            return None
        with _cycle_check(renderer, prove_interior):
            _check(renderer, renderer.RenderExact(iter_bytes, F, L, cx, cy, bailout, inclusive, cap), "fs_render_exact")
    return _proved(renderer).reshape(cy.shape[1], cx.shape[1]) if prove_interior else None


class _periods:
    """The period planes on for the duration of a call, off again behind it."""

    def __init__(self, renderer):
        self.renderer = renderer

    def __enter__(self):
        _check(self.renderer, self.renderer.SetExactPeriods(True), "fs_set_exact_periods")

    def __exit__(self, *exc):
        self.renderer.SetExactPeriods(False)


def render_periods(renderer, view, bailout=4, frac_bits=None, iter_bytes=4, inclusive=False, prove_interior=False, cap=None):
    """render with the period planes (fs_set_exact_periods; DESIGN.md 6.3 "Period planes"): the exact family's own period map, at any
    depth up to 24 limbs with no reference orbit.  Returns (frame, atom) or, with prove_interior, (frame, atom, cycle_length), numpy
    arrays [H, W]: the frame as read from the iteration buffer -- byte for byte render's -- the atom period of every pixel (uint64:
    the index n at which |z_n| is smallest among the states that passed the escape test within the cap, ties to the earliest; 0 where
    c itself escapes) and the cycle length of every pixel the cycle check proved (uint64, 0 elsewhere; a multiple of the cycle's
    period).  cap: in place of view.num_iterations.  Not the Feature Finder's trigger: see features.period_map / pt_grid for that."""
    F = view.precision_bits + GUARD_BITS if frac_bits is None else int(frac_bits)
    if uses_wide(limbs_for(F)):
        raise ValueError("render_periods: %d fractional bits need more than %d limbs; the wide path has no period planes" % (F, MAX_LIMBS))
    cap = view.num_iterations if cap is None else int(cap)
    with _periods(renderer):
        render(renderer, view, bailout, F, iter_bytes, inclusive, prove_interior, n_iterations=cap)
    h, w = renderer.GetHeight(), renderer.GetWidth()
    out = renderer.new_iter_buffer()
    _check(renderer, renderer.RenderCurrent(cap, out), "fs_render_current")
    _check(renderer, renderer.SyncComputeStream(), "fs_sync_compute")
    err, atom = renderer.ExactAtomPeriods()
    _check(renderer, err, "fs_read_exact_atom_periods")
    planes = (out[:h, :w].copy(), atom.reshape(h, w))
    if prove_interior:
        err, lengths = renderer.ExactCycleLengths()
        _check(renderer, err, "fs_read_exact_cycle_lengths")
        planes += (lengths.reshape(h, w),)
    return planes


def continue_render(renderer, n_iterations):
    """The kept frame in the iteration buffer raised to the cap n_iterations (fs_render_exact_continue): afterwards the buffer is
    what render writes with that cap, and the kept set is that cap's, so calls chain.  Path, number format, bailout and cycle check
    are the kept set's; nothing is chosen here.  Returns what render returns: bool[H, W] of the proved samples when the kept render
    ran with prove_interior, else None."""
    _check(renderer, renderer.RenderExactContinue(n_iterations), "fs_render_exact_continue")
    if not renderer.ExactKept()["cycle_check"]:
        return None
    return _proved(renderer).reshape(renderer.GetHeight(), renderer.GetWidth())


def render_progressive(renderer, view, caps, bailout=4, frac_bits=None, iter_bytes=4, inclusive=False, prove_interior=False):
    """A generator: the view's exact frame at every cap of `caps`, in ascending order, each step resuming the samples the one
    before left at its cap.  Yields (cap, what render returns) with that cap's frame in the iteration buffer -- a valid frame for
    RenderCurrent, autozoom and audit, equal to render's at that cap.  The kept set is dropped when the generator ends."""
    caps = sorted(int(c) for c in caps)
    try:
        for k, cap in enumerate(caps):
            if k == 0:
                yield cap, render(renderer, view, bailout, frac_bits, iter_bytes, inclusive, prove_interior, keep=True, n_iterations=cap)
            else:
                yield cap, continue_render(renderer, cap)
    finally:
        renderer.DropExactKept()


def uses_wide(limbs):
    """The dispatch rule of render: the wide kernel exactly where the narrow one has no instantiation."""
    return int(limbs) > MAX_LIMBS


def sample_counts(renderer, view, xs, ys, bailout=4, frac_bits=None, levels=(), inclusive=False):
    """(values int64[n], stable bool[n, len(levels)]): min(E - 1, view.num_iterations) of the samples (xs[i], ys[i]) of the
    view's antialiased frame, and per ladder level whether the value is the same at c +- s and c +- is, s = the frame's width /
    2^level (the stability bits of the exact-count fixture).  One wave per sample at any limb count up to 704
    (fs_exact_sample_counts); needs no InitializeMemory."""
    F = view.precision_bits + GUARD_BITS if frac_bits is None else int(frac_bits)
    L = limbs_for(F)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)

    def run(ax, ay):
        err, out = renderer.ExactSampleCounts(F, L, ax[:, xs], ay[:, ys], bailout, inclusive, view.num_iterations)
        _check(renderer, err, "fs_exact_sample_counts")
        return out.astype(np.int64)

    cx, cy = axes(view, F, limbs=L)
    values = run(cx, cy)
    stable = np.ones((len(xs), len(levels)), bool)
    for j, level in enumerate(levels):
        cx3, cy3 = axes(view, F, level=level, limbs=L)
        for ax, ay in ((cx3[1], cy3[0]), (cx3[2], cy3[0]), (cx3[0], cy3[1]), (cx3[0], cy3[2])):  # c + s, c - s, c + is, c - is
            stable[:, j] &= run(ax, ay) == values
    return values, stable


def _to_limbs(values, limbs):
    """uint32[limbs, n]: Python integers as two's-complement numbers of `limbs` limbs, limb-major."""
    mask = (1 << (32 * limbs)) - 1
    raw = b"".join((int(v) & mask).to_bytes(4 * limbs, "little") for v in values)
    return np.ascontiguousarray(np.frombuffer(raw, "<u4").reshape(len(values), limbs).T)


def _from_limbs(arr):
    """Python integers of a limb-major uint32[limbs, n], two's complement."""
    limbs = arr.shape[0]
    raw = np.ascontiguousarray(arr.T.astype("<u4")).tobytes()
    return [int.from_bytes(raw[4 * limbs * i:4 * limbs * (i + 1)], "little", signed=True) for i in range(arr.shape[1])]


def points(values, frac_bits, limbs=None):
    """(ints, array): floor(value * 2^frac_bits) of every value -- decimal strings or Fractions, read as exact rationals -- as Python
    integers and as the limb-major uint32[limbs, n] the exact entry points take (limbs defaults to limbs_for(frac_bits))."""
    from fractions import Fraction
    F = int(frac_bits)
    limbs = limbs_for(F) if limbs is None else int(limbs)
    ints = []
    for v in values:
        q = Fraction(v)
        ints.append((q.numerator << F) // q.denominator)
    for v in ints:
        if not -(1 << (32 * limbs - 1)) <= v < 1 << (32 * limbs - 1):
            raise ValueError("points: a value does not fit %d limbs at %d fractional bits" % (limbs, F))
    return ints, _to_limbs(ints, limbs)


def eval_points(renderer, cxs, cys, lengths, frac_bits, bailout=256, inclusive=False, wide=False):
    """Point runs on the GPU (fs_exact_eval_points; DESIGN.md 6.3 "Point runs"): run e iterates c = (cxs[e] + i cys[e]) / 2^frac_bits
    -- Python integers -- from z_1 = c up to n = lengths[e].  Returns (values, atoms, ends), lists of Python integers:
    values[e] = v = min(E - 1, lengths[e]); atoms[e] = the n in 1 .. v with the smallest x_n^2 + y_n^2, the earliest on ties, 0 when
    v = 0; ends[e] = (x_p, y_p) * 2^frac_bits at p = lengths[e] when v == p, else None.  Equal to the recurrence on Python integers.
    Up to 758 fractional bits (24 limbs) a lane holds a run; ValueError beyond.  wide=True: a wave holds a run at every limb count
    (fs_exact_eval_points_wide), up to 22 518 fractional bits (704 limbs), ValueError beyond; the results are the same wherever both
    run."""
    F = int(frac_bits)
    L = limbs_for(F)
    if wide and L > MAX_WIDE_LIMBS:
        raise ValueError("eval_points: %d fractional bits need more than %d limbs" % (F, MAX_WIDE_LIMBS))
    if not wide and uses_wide(L):
        raise ValueError("eval_points: %d fractional bits need more than %d limbs; wide=True runs them on the wide path" % (F, MAX_LIMBS))
    cxs, cys, lengths = list(cxs), list(cys), [int(p) for p in lengths]
    if not (len(cxs) == len(cys) == len(lengths)):
        raise ValueError("eval_points: cxs, cys and lengths must have one length")
    if not cxs:
        return [], [], []
    call = renderer.ExactEvalPointsWide if wide else renderer.ExactEvalPoints
    err, values, atoms, end_x, end_y = call(F, L, _to_limbs(cxs, L), _to_limbs(cys, L), np.array(lengths, np.uint64), bailout, inclusive)
    _check(renderer, err, "fs_exact_eval_points_wide" if wide else "fs_exact_eval_points")
    values, atoms = [int(v) for v in values], [int(a) for a in atoms]
    xs, ys = _from_limbs(end_x), _from_limbs(end_y)
    return values, atoms, [(x, y) if v == p else None for x, y, v, p in zip(xs, ys, values, lengths)]


def refine_points(evaluate, c0s, deltas, periods, frac_bits, rounds=16):
    """Found points to nuclei by a derivative-free secant iteration on z_p(c), on Python integers (DESIGN.md 6.3 "Point runs").
    evaluate(cxs, cys, lengths) -> (values, atoms, ends) is eval_points' contract with the renderer bound (or any model of it);
    c0s = [(cx, cy)] as integers c * 2^frac_bits, deltas = the real offset of every point's second starting point, periods = p.
    Every round puts all points still running into ONE evaluate call; the first call holds both starting points of every point.
    Per point (`//` and `>>` floor):
        c1 = c0 + (delta, 0); either start short of p: "escaped", no result
        at most `rounds` times: d = f1 - f0 (the endpoints); d == 0: "stalled"
            q = floor(f1 conj(d) 2^F / |d|^2), s = (q (c1 - c0)) >> F, c2 = c1 - s; c2 == c1: "fixed"
            evaluate c2; short of p: "escaped"; else (c0, f0, c1, f1) = (c1, f1, c2, f2)
        otherwise "rounds"
    Returns one dict per point: status; c = (cx, cy) of the evaluated iterate with the smallest |z_p|, the earliest on ties (None
    when no iterate reached p); atom = the atom period there; converged = atom == p; evaluations; log2 = log2 |z_p| of every iterate
    that reached p, in order (floats, for reading only)."""
    import math
    F = int(frac_bits)
    n = len(c0s)
    periods = [int(p) for p in periods]
    c0 = [(int(c[0]), int(c[1])) for c in c0s]
    c1 = [(c[0] + int(d), c[1]) for c, d in zip(c0, deltas)]
    status, n_eval = [None] * n, [2] * n
    evals = [[] for _ in range(n)]  # (c, atom, endpoint) of every iterate that reached p

    def run(items):
        """items = [(point, c)]: one evaluate call; the endpoint (or None) per item."""
        values, atoms, ends = evaluate([c[0] for _, c in items], [c[1] for _, c in items], [periods[k] for k, _ in items])
        out = []
        for (k, c), v, a, end in zip(items, values, atoms, ends):
            reached = int(v) == periods[k] and end is not None
            if reached:
                evals[k].append((c, int(a), (int(end[0]), int(end[1]))))
            out.append(evals[k][-1][2] if reached else None)
        return out

    f0, f1 = [None] * n, [None] * n
    if n:
        first = run([(k, c0[k]) for k in range(n)] + [(k, c1[k]) for k in range(n)])
        f0, f1 = first[:n], first[n:]
    short_start = {k for k in range(n) if f0[k] is None or f1[k] is None}
    for k in short_start:
        status[k] = "escaped"
    for _ in range(int(rounds)):
        items = []
        for k in range(n):
            if status[k] is not None:
                continue
            dx, dy = f1[k][0] - f0[k][0], f1[k][1] - f0[k][1]
            if dx == 0 and dy == 0:
                status[k] = "stalled"
                continue
            dd = dx * dx + dy * dy
            qx = ((f1[k][0] * dx + f1[k][1] * dy) << F) // dd
            qy = ((f1[k][1] * dx - f1[k][0] * dy) << F) // dd
            ex, ey = c1[k][0] - c0[k][0], c1[k][1] - c0[k][1]
            c2 = (c1[k][0] - ((qx * ex - qy * ey) >> F), c1[k][1] - ((qx * ey + qy * ex) >> F))
            if c2 == c1[k]:
                status[k] = "fixed"
                continue
            items.append((k, c2))
        if not items:
            break
        for (k, c2), f2 in zip(items, run(items)):
            n_eval[k] += 1
            if f2 is None:
                status[k] = "escaped"
            else:
                c0[k], f0[k], c1[k], f1[k] = c1[k], f1[k], c2, f2
    out = []
    for k in range(n):
        norm = lambda e: e[2][0] * e[2][0] + e[2][1] * e[2][1]
        res = {"status": status[k] or "rounds", "c": None, "atom": None, "converged": False, "evaluations": n_eval[k],
               "log2": [0.5 * math.log2(norm(e)) - F if norm(e) else -math.inf for e in evals[k]]}
        if k not in short_start:
            best = min(range(len(evals[k])), key=lambda j: (norm(evals[k][j]), j))
            res["c"], res["atom"] = evals[k][best][0], evals[k][best][1]
            res["converged"] = res["atom"] == periods[k]
        out.append(res)
    return out


def lattice(view, cols, rows):
    """(xs, ys) = uint32[n] each: `cols` x `rows` samples spread evenly over the view's antialiased frame, the first and the last
    row and column included, row-major (rounded positions that coincide are taken once)."""
    w, h = view.width * view.antialiasing, view.height * view.antialiasing
    ax = np.unique(np.round(np.linspace(0, w - 1, cols)).astype(np.int64))
    ay = np.unique(np.round(np.linspace(0, h - 1, rows)).astype(np.int64))
    gx, gy = np.meshgrid(ax, ay)
    return gx.ravel().astype(np.uint32), gy.ravel().astype(np.uint32)


MIN_STABLE_SAMPLES, MIN_STABLE_SHARE = 100, 0.2  # the floors a stable set must meet to carry a verdict


class AuditReport:
    """What fs_exact_audit says about a frame.  The record's fields: n_samples, n_levels, n_equal, n_differ, n_capped,
    n_offenders, and per level, in the order of `levels`, stable_count (the record's stable[]), stable_differ, stable_capped and
    max_abs_diff; `record` is the _capi.AuditResult itself.  Per sample: values (the exact counts, int64[n]), frame_values
    (int64[n]) and stable (bool[n, len(levels)]).  offenders: the first (at most 16) differing samples in sample order, as dicts
    {sample, x, y, frame_value, exact_value, stable: [bool per level]}.  With audit(prove_interior=True): n_proved, how many of the
    samples' own runs (at c) the cycle check finished by proof, and proved (bool[n]), which; 0 and None otherwise."""

    def __init__(self, levels, n_samples, stable_count, stable_differ, stable_capped=None, max_abs_diff=None, n_equal=0, n_differ=0,
                 n_capped=0, offenders=(), values=None, frame_values=None, stable=None, record=None, n_proved=0, proved=None):
        k = len(levels)
        ints = lambda a: [int(v) for v in (a if a is not None else [0] * k)]
        self.levels, self.n_samples, self.n_levels = tuple(int(lv) for lv in levels), int(n_samples), k
        self.stable_count, self.stable_differ = ints(stable_count), ints(stable_differ)
        self.stable_capped, self.max_abs_diff = ints(stable_capped), ints(max_abs_diff)
        self.n_equal, self.n_differ, self.n_capped = int(n_equal), int(n_differ), int(n_capped)
        self.offenders = list(offenders)
        self.n_offenders = len(self.offenders)
        self.values, self.frame_values, self.stable, self.record = values, frame_values, stable, record
        self.n_proved, self.proved = int(n_proved), proved

    def finest_clean_level(self, min_samples=MIN_STABLE_SAMPLES, min_share=MIN_STABLE_SHARE):
        """The finest level (the largest k of s = width / 2^k) at which the frame misses on no stable sample and whose stable set
        holds at least min_samples samples and min_share of all samples; None when there is none."""
        clean = [lv for lv, n, bad in zip(self.levels, self.stable_count, self.stable_differ)
                 if bad == 0 and n >= min_samples and n >= min_share * self.n_samples]
        return max(clean) if clean else None

    def as_dict(self):
        """The record as plain Python values (what tools/audit_frame.py prints)."""
        return {"levels": list(self.levels), "n_samples": self.n_samples, "n_equal": self.n_equal, "n_differ": self.n_differ,
                "n_capped": self.n_capped, "stable": self.stable_count, "stable_differ": self.stable_differ,
                "stable_capped": self.stable_capped, "max_abs_diff": self.max_abs_diff}


def audit(renderer, view, xs, ys, levels=(), bailout=256, frac_bits=None, inclusive=False, device_iters=None, prove_interior=False):
    """The frame in the renderer's iteration buffer (or device_iters: another device buffer of its geometry) against the exact
    counts min(E - 1, view.num_iterations) at the samples (xs[i], ys[i]) of the view's antialiased frame, with the stability of
    every sample at the ladder `levels` (at most 8; s = the frame's width / 2^level): an AuditReport.  One call (fs_exact_audit):
    all len(xs) * (1 + 4 len(levels)) runs advance as one list on the device, the frame is read next to them, and only the record
    and three small per-sample arrays come back.  The frame's rule must be min(E - 1, N): the perturbation kernels (bailout 256)
    and the direct kernels with a CPU twin (bailout 4), not the low-precision direct kernels.
    prove_interior: the cycle check is on for the call (up to 24 limbs; beyond, it is ignored); the report is the same but for
    n_proved and proved, and renderer.ExactProved(len(xs) * (1 + 4 len(levels))) holds the proved mask of all runs."""
    F = view.precision_bits + GUARD_BITS if frac_bits is None else int(frac_bits)
    L = limbs_for(F)
    levels = tuple(int(lv) for lv in levels)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    cx, cy = axes(view, F, limbs=L)
    cx_runs, cy_runs = [cx[:, xs]], [cy[:, ys]]
    for level in levels:
        cx3, cy3 = axes(view, F, level=level, limbs=L)
        for ax, ay in ((cx3[1], cy3[0]), (cx3[2], cy3[0]), (cx3[0], cy3[1]), (cx3[0], cy3[2])):  # c + s, c - s, c + is, c - is
            cx_runs.append(ax[:, xs])
            cy_runs.append(ay[:, ys])
    proving = bool(prove_interior) and not uses_wide(L) and len(xs) > 0
    with _cycle_check(renderer, proving):
        err, res, values, frame_values, bits = renderer.ExactAudit(F, L, xs, ys, np.stack(cx_runs), np.stack(cy_runs), bailout,
                                                                   inclusive, view.num_iterations, device_iters=device_iters)
    _check(renderer, err, "fs_exact_audit")
    proved = _proved(renderer, len(xs) * (1 + 4 * len(levels)))[:len(xs)] if proving else None
    k = len(levels)
    stable = ((bits[:, None] >> np.arange(k, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(len(xs), k)
    offenders = [{"sample": int(o.sample), "x": int(xs[o.sample]), "y": int(ys[o.sample]), "frame_value": int(o.frame_value),
                  "exact_value": int(o.exact_value), "stable": [bool((o.stable_bits >> j) & 1) for j in range(k)]}
                 for o in res.offenders[:res.n_offenders]]
    return AuditReport(levels, res.n_samples, res.stable[:k], res.stable_differ[:k], res.stable_capped[:k], res.max_abs_diff[:k],
                       res.n_equal, res.n_differ, res.n_capped, offenders, values.astype(np.int64), frame_values.astype(np.int64),
                       stable, res, n_proved=0 if proved is None else int(proved.sum()), proved=proved)


def stable_mask(renderer, view, level, bailout=4, frac_bits=None, prove_interior=False):
    """bool[H, W]: the pixels of the exact frame in the iteration buffer (exact.render of the same view, bailout and frac_bits,
    strict) whose count is the same at c +- s and c +- is, s = the frame's width / 2^level.  prove_interior: the four shifted
    frames are rendered with the cycle check on; the mask is the same."""
    F = view.precision_bits + GUARD_BITS if frac_bits is None else int(frac_bits)
    L = limbs_for(F)
    cx3, cy3 = axes(view, F, level=level, limbs=L)
    with _cycle_check(renderer, prove_interior):
        err, mask = renderer.ExactStableMask(F, L, cx3, cy3, bailout, view.num_iterations)
    _check(renderer, err, "fs_exact_stable_mask")
    return mask.astype(bool)


__all__ = ["GUARD_BITS", "MAX_FRAC_BITS", "MAX_WIDE_LIMBS", "MAX_WIDE_FRAC_BITS", "limbs_for", "axes", "render", "render_periods",
           "continue_render",
           "render_progressive", "uses_wide",
           "sample_counts", "points", "eval_points", "refine_points", "stable_mask", "lattice", "audit", "AuditReport"]
