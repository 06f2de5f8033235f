"""The exact renderer: fixed-point escape counts at any depth on the GPU, with no reference orbit and no rounding.

The render path of the reference's CpuHigh (CalcCpuHDR<IterType, HighPrecision, double>, Fractal.cpp:1200-1201, 2096-2206): every
sample is iterated by itself in high precision.  Here that is integer arithmetic on 32-bit limbs (csrc/exact_math.hpp,
csrc/kernels_exact.hip): x' = floor((x^2 - y^2) / 2^F) + cx, y' = floor(2xy / 2^F) + cy, escape when x^2 + y^2 > R 2^2F.  The frame
equals GMP integer iteration of that recurrence on every pixel, and is an ordinary frame in the renderer's iteration buffer:
min(E - 1, N) like every other path.  The axes come from the view's bounding-box strings read as exact rationals
(fsh_view_exact_axes).
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


def render(renderer, view, bailout=4, frac_bits=None, iter_bytes=4, inclusive=False):
    """The view's exact frame into the renderer's iteration buffer (InitializeMemory with the view's antialiased size and
    iter_bytes comes first), view.num_iterations the cap.  frac_bits defaults to view.precision_bits + 64.  Has the shape
    autozoom.zoom wants for its `render` argument.  Up to 24 limbs (758 bits) a lane holds a sample (fs_render_exact); beyond, a
    wave does (fs_render_exact_wide), up to 704 limbs."""
    F = view.precision_bits + GUARD_BITS if frac_bits is None else int(frac_bits)
    L = limbs_for(F)
    cx, cy = axes(view, F, limbs=L)
    if uses_wide(L):
        _check(renderer, renderer.RenderExactWide(iter_bytes, F, L, cx, cy, bailout, inclusive, view.num_iterations),
               "fs_render_exact_wide")
    else:
        _check(renderer, renderer.RenderExact(iter_bytes, F, L, cx, cy, bailout, inclusive, view.num_iterations), "fs_render_exact")


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


def stable_mask(renderer, view, level, bailout=4, frac_bits=None):
    """bool[H, W]: the pixels of the exact frame in the iteration buffer (exact.render of the same view, bailout and frac_bits,
    strict) whose count is the same at c +- s and c +- is, s = the frame's width / 2^level."""
    F = view.precision_bits + GUARD_BITS if frac_bits is None else int(frac_bits)
    L = limbs_for(F)
    cx3, cy3 = axes(view, F, level=level, limbs=L)
    err, mask = renderer.ExactStableMask(F, L, cx3, cy3, bailout, view.num_iterations)
    _check(renderer, err, "fs_exact_stable_mask")
    return mask.astype(bool)


__all__ = ["GUARD_BITS", "MAX_FRAC_BITS", "MAX_WIDE_LIMBS", "MAX_WIDE_FRAC_BITS", "limbs_for", "axes", "render", "uses_wide",
           "sample_counts", "stable_mask"]
