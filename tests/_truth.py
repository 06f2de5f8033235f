"""Exact escape counts (tests/truth/exact_counts.cpp) and the rules that turn them into what each render path must
output -- test infrastructure only.

"Pinned by exact counts": on samples whose exact count does not change when c moves by a stated fraction of the frame
width (the stability level), a path's output must EQUAL the value its rule derives from the exact count.  The level of a
mantissa width is chosen per fixture case against the reference-pinned oracle of that width (make_exact_counts.py) and
stored in the fixture; an unpinned path of the same width and mode is held to equality at that same level.

The exact count E_R of a sample is the first n >= 1 with |z_n|^2 > R under z_0 = 0, z_1 = c, z_{n+1} = z_n^2 + c, or 0 when
there is none with n <= cap + 1.  Rules (N = the iteration cap):

  perturbation paths, R = 256 -- CalcCpuPerturbationFractalBLA (Fractal.cpp:2266-2470) and CalcCpuPerturbationFractalLAV2
    (:2545-2678) start at z_0 (DeltaSubN = 0, iter = 0), step, test |z_{iter+1}|^2 > 256 and only then count the step:
    an escape at n leaves iter = n - 1; without one the loop ends at iter = N.          expected = min(E_256 - 1, N)
  CPU direct paths, R = 4 -- CalcCpuHDR (Fractal.cpp:2096-2206) starts at z = c = z_1 with i = 0 and tests |z_{i+1}|^2 > 4
    before stepping: the same offset.                                                   expected = min(E_4 - 1, N)
  low-precision GPU direct kernels, R = 4 -- mandel_1x_float / mandel_2x_float / mandel_2x_double
    (LowPrecisionKernels.cuh:682-777, :384-555, :171-290) start at z_0 = 0 with iter = 0 and run `while (|z_iter|^2 < 4 &&
    iter < n)`, iter += iteration_precision: iter is the first multiple of ip at or above E_4.  They sample output row r
    at cy + dy * (height - 1 - r) with cy = minY, which is sample row r + 1 of the map above (the row shift).
                                                                   expected = min(roundup(E_4, ip), roundup(n, ip))
    with n = N - (ip - 1) for 1x32 (:700) and N for the others.
"""
import ctypes as C
import json
import os
import subprocess
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TRUTH_DIR = os.path.join(HERE, "truth")
FIXTURE = os.path.join(HERE, "golden", "exact_counts.json")

# stability ladder: a sample is stable at level k when its exact count is the same at c +- W/2^k and c +- i W/2^k, W the
# frame width.  Steps of 2^-5 from 2^-10 to 2^-35, plus 2^-17 and 2^-22.  Those two were added after the first run: with
# steps of 2^-5 HDRFloat<float>'s finest miss-free level was 2^-15 on the shallow views, where 18 - 25 % of the samples are
# stable -- at or under the 20 % floor -- while it already missed at 2^-20.  The level is still chosen by the pinned path and
# the floors are unchanged; the ladder is only finer where that width's transition lies.
LADDER = (10, 15, 17, 20, 22, 25, 30, 35)
GUARD_BITS = 64
# section "the condition each comparison uses": the stable set a comparison rests on must not be small
MIN_STABLE_SHARE = 0.20
MIN_STABLE_SAMPLES = 100

_lib = None


def lib():
    """g++ build of tests/truth/exact_counts.cpp against the GMP that libfsinputs links."""
    global _lib
    if _lib is None:
        from fractalshark_amd import _build
        so = os.path.join(TRUTH_DIR, "libexact_counts.so")
        src = os.path.join(TRUTH_DIR, "exact_counts.cpp")
        if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
            gmp = _build.GMP_PREFIX
            subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(gmp, "include"), "-o", so, src,
                            "-L" + os.path.join(gmp, "lib"), "-lgmp", "-Wl,-rpath," + os.path.join(gmp, "lib"), "-lpthread"],
                           check=True)
        h = C.CDLL(so)
        h.exc_exact_counts.restype = C.c_int
        h.exc_exact_counts.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int]
        _lib = h
    return _lib


def exact_counts(bbox, w, h, xs, ys, limit, R, frac_bits, shifts=LADDER, inclusive=False, threads=16):
    """(counts uint64[n], stable bool[n, len(shifts)]) for the samples (xs[i], ys[i]) of a w x h frame over bbox =
    [minX, minY, maxX, maxY] (decimal strings).  counts = first n <= limit with |z_n|^2 > R (>= R if inclusive), 0 = none."""
    xs, ys = np.ascontiguousarray(xs, np.uint32), np.ascontiguousarray(ys, np.uint32)
    sh = np.ascontiguousarray(shifts, np.int32)
    counts = np.zeros(len(xs), np.uint64)
    stable = np.zeros((len(xs), max(1, len(sh))), np.uint8)
    bb = (C.c_char_p * 4)(*[s.encode() for s in bbox])
    r = Fraction(R)
    rc = lib().exc_exact_counts(bb, w, h, xs.ctypes.data, ys.ctypes.data, len(xs), int(limit), r.numerator, r.denominator,
                                1 if inclusive else 0, int(frac_bits), sh.ctypes.data, len(sh), counts.ctypes.data,
                                stable.ctypes.data, min(16, int(threads)))
    if rc != 0:
        raise ValueError("exact_counts could not read the bounding box %r" % (bbox,))
    return counts, stable[:, :len(sh)].astype(bool)


def python_exact_count(bbox, w, h, x, y, limit, R, frac_bits, inclusive=False):
    """The same count from Python integers: the second, independent implementation that guards the counter."""
    minx, miny, maxx, maxy = (Fraction(s) for s in bbox)
    F = frac_bits
    fix = lambda q: (q.numerator << F) // q.denominator
    cx, cy = fix(minx + (maxx - minx) * x / w), fix(maxy - (maxy - miny) * y / h)
    bail = fix(Fraction(R)) << F
    zx, zy = cx, cy
    for n in range(1, limit + 1):
        xx, yy = zx * zx, zy * zy
        if xx + yy > bail or (inclusive and xx + yy == bail):
            return n
        zx, zy = ((xx - yy) >> F) + cx, ((2 * zx * zy) >> F) + cy
    return 0


def lattice_axes(w, h, cols, rows):
    """Sampled columns and rows: `cols` x `rows` spread evenly over the whole w x h frame, first and last of each included
    (row 0 and column 0 hold the origin of the pixel map, the last ones the far edge)."""
    xs = np.unique(np.round(np.linspace(0, w - 1, cols)).astype(np.int64))
    ys = np.unique(np.round(np.linspace(0, h - 1, rows)).astype(np.int64))
    return xs, ys


def lattice(w, h, cols, rows):
    """The samples of lattice_axes, row-major: (xs[i], ys[i])."""
    xs, ys = lattice_axes(w, h, cols, rows)
    gx, gy = np.meshgrid(xs, ys)
    return gx.ravel().astype(np.uint32), gy.ravel().astype(np.uint32)


def sample_rows(render_rows, w, xs, ys, workers=8):
    """What a row renderer gives at the samples: render_rows(y0, y1) -> padded frame buffer with rows [y0, y1) filled.  Each
    sampled row is rendered by itself (one oracle thread each, `workers` rows at a time), never the whole frame.  The first row
    is rendered before the pool starts, so that anything a renderer builds on its first call is built by one thread."""
    from concurrent.futures import ThreadPoolExecutor
    rows = sorted(set(int(y) for y in ys))
    one = lambda y: np.array(render_rows(y, y + 1)[y, :w])
    got = {rows[0]: one(rows[0])}
    with ThreadPoolExecutor(workers) as ex:
        got.update(zip(rows[1:], ex.map(one, rows[1:])))
    return np.array([got[int(y)][int(x)] for x, y in zip(xs, ys)], np.int64)


# ---- exact count -> expected output
def expect_minus_one(E, cap):
    """Perturbation paths (R = 256) and CPU direct paths (R = 4): min(E - 1, N); no escape within N + 1 -> N."""
    E = np.asarray(E, np.int64)
    return np.where(E == 0, cap, np.minimum(E - 1, cap))


def expect_lp_direct(E, cap, ip, kind):
    """Low-precision GPU direct kernels (R = 4; they bail at >= 4, which only the boundary samples can tell): the first multiple of ip at or above E, the loop bound likewise."""
    E = np.asarray(E, np.int64)
    n = cap - (ip - 1) if kind == "1x32" else cap
    up = lambda v: (v + ip - 1) // ip * ip
    return np.where(E == 0, up(n), np.minimum(up(E), up(n)))


# ---- strict or inclusive bailout: exactly representable boundary samples
# An 8 x 8 view over [-2, 2]^2: dx = dy = 1/2, every c a multiple of 1/2 and exact in every type under test.  Sample (4, 0) is
# c = 2i: |z_1|^2 = 4 exactly, z_2 = -4 + 2i.  Sample (0, 4) is c = -2: z_n = 2 and |z_n|^2 = 4 for every n >= 2.  A path that
# bails at |z|^2 > 4 counts them as E = 2 and "never"; one that bails at >= 4 as E = 1 and 1.  No stability argument applies or is
# needed: all the arithmetic on these two orbits is exact.  The low-precision direct kernels render c = -2i at (4, row 7) and
# c = -2 at (0, row 3) (their row r is sample row r + 1).
# For a perturbation path the sample has to be the reference point itself (delta c = 0, so that the pixel's orbit IS the stored
# orbit and nothing is rounded): the centre (4, 4) of an 8 x 8 view over [-20, -12] x [-4, 4] is c = -16 with |z_1|^2 = 256
# exactly and z_2 = 240 (R = 256: strict E = 2, inclusive E = 1); the centre of one over [-4, 0] x [-2, 2] is c = -2 (R = 4: strict
# never, inclusive E = 1), for the HDRFloat<CudaDblflt> kernel whose bailout is at 4.
BOUNDARY_BBOX, BOUNDARY_SIZE, BOUNDARY_CAP = ("-2", "-2", "2", "2"), 8, 64
BOUNDARY_SAMPLES = ((4, 0), (0, 4))      # (x, y) in the CPU paths' map
BOUNDARY_SAMPLES_LP = ((4, 7), (0, 3))   # (x, output row) of the low-precision direct kernels: c = -2i, c = -2
# mandel_1x_float / 2x_float / 2x_double loop `while (|z|^2 < 4 ...)` and so stop AT 4; mandel_4x_float / 4x_double loop
# `while (zrsqr + zisqr <= 4.0 ...)` (LowPrecisionKernels.cuh:5-75, :77-140) and stop only ABOVE it
LP_BAILS_AT_EQUALITY = {"1x32": True, "2x32": True, "2x64": True, "4x32": False, "4x64": False}


BOUNDARY_BBOX_256, BOUNDARY_BBOX_CENTRE_4, BOUNDARY_CENTRE = ("-20", "-4", "-12", "4"), ("-4", "-2", "0", "2"), (4, 4)


def boundary_view(inputs, bbox=BOUNDARY_BBOX):
    return inputs.View(*bbox, BOUNDARY_SIZE, BOUNDARY_SIZE, num_iterations=BOUNDARY_CAP)


def boundary_centre_count(v, R, inclusive):
    """Exact count of the centre sample of a boundary view."""
    E, _ = exact_counts(v.bbox(), BOUNDARY_SIZE, BOUNDARY_SIZE, [BOUNDARY_CENTRE[0]], [BOUNDARY_CENTRE[1]], BOUNDARY_CAP + 1, R,
                        v.precision_bits + GUARD_BITS, shifts=[], inclusive=inclusive)
    return E.astype(np.int64)


def boundary_counts(v, inclusive):
    """Exact counts of the two boundary samples (the conjugate c = -2i has c = 2i's count)."""
    xs, ys = zip(*BOUNDARY_SAMPLES)
    E, _ = exact_counts(v.bbox(), BOUNDARY_SIZE, BOUNDARY_SIZE, xs, ys, BOUNDARY_CAP + 1, 4, v.precision_bits + GUARD_BITS,
                        shifts=[], inclusive=inclusive)
    return E.astype(np.int64)


# ---- fixture
_fx = None


def fixture():
    global _fx
    if _fx is None:
        with open(FIXTURE) as f:
            _fx = json.load(f)
    return _fx


class Case:
    """One fixture case: samples, exact counts per R, stability bits, and the levels the pinned oracles chose."""

    def __init__(self, name, entry=None):
        """The committed case `name`, or (the generator, for the entry it is building) the given entry."""
        c = fixture()["cases"][name] if entry is None else entry
        self.name, self.raw = name, c
        self.w, self.h, self.aa, self.cap = c["width"], c["height"], c["aa"], c["cap"]
        gx, gy = np.meshgrid(np.array(c["columns"], np.int64), np.array(c["rows"], np.int64))
        self.xs, self.ys = gx.ravel(), gy.ravel()  # row-major over the sampled rows x columns
        self.ladder = tuple(c["ladder"])
        self.levels = c["levels"]

    def counts(self, R):
        """E_R per sample (strict: |z_n|^2 > R).  Whether a path bails at > R or at >= R makes no difference on a stable sample
        (one with |z_n|^2 == R exactly never is); that is checked on exactly representable boundary samples instead
        (BOUNDARY below)."""
        return np.array(self.raw["R%d" % R]["counts"], np.int64)

    def stable(self, R, level):
        bits = np.array(self.raw["R%d" % R]["stable_bits"], np.int64)
        return ((bits >> self.ladder.index(level)) & 1).astype(bool)

    def approx_level(self, m):
        """The level for a path of mantissa class m ("m24" | "m53") that really takes LA steps.  On the generated shallow views
        the pinned CPU LAv2 function takes next to none (its zero-with-exponent-0 start value makes every LA step unusable,
        tests/test_plain_oracle.py), so its level there is perturbation-only's; LA and BLA steps are both linear approximations
        accepted inside a validity radius, and the pinned evidence for such a path at this width is the BLA function.  The
        coarser of the two pinned approximating levels is used; None unless both carry a comparison."""
        lv = [self.levels.get(k, {}) for k in (m + "_lav2_gpustage", m + "_bla")]
        return min(l["level"] for l in lv) if all(l.get("carries") for l in lv) else None

    def view(self, inputs):
        if "view" in self.raw:
            return inputs.View.builtin(self.raw["view"], self.w // self.aa, self.h // self.aa, antialiasing=self.aa)
        b = self.raw["bbox"]
        v = inputs.View(b[0], b[1], b[2], b[3], self.w // self.aa, self.h // self.aa, num_iterations=self.cap,
                        antialiasing=self.aa)
        return v

    def sample(self, frame, row_shift=0):
        return np.asarray(frame)[self.ys - row_shift, self.xs].astype(np.int64)


def carries(name, key):
    """Whether the pinned path `key` chose, for this case, a level whose stable set meets both floors (all samples stable at the
    level, capped ones included: the same set `misses` asserts the floors on).  Where it does not, no comparison of that mantissa width and mode rests on the case; the pairs
    concerned are listed in tests/test_exact_counts.py::test_which_pinned_paths_carry_no_comparison."""
    lv = fixture()["cases"].get(name, {}).get("levels", {}).get(key)
    return bool(lv and lv["carries"])


def meets_floors(n_stable, n_samples):
    """The one definition of the floors: at least 100 stable samples (capped ones included) and 20 % of the case's samples."""
    return bool(n_stable >= MIN_STABLE_SAMPLES and n_stable >= MIN_STABLE_SHARE * n_samples)


def misses(case, got, expected, R, level, mask=None):
    """Compare at a level: every sample stable at `level` (capped ones included: their expected value is the cap's) must be
    equal.  mask = samples the path has an output for (the others leave the stable set).  Returns (number of misses, stable
    count, share of the case's samples); asserts the two floors on the stable set."""
    st = case.stable(R, level)
    if mask is not None:
        st = st & mask
    n, share = int(st.sum()), float(st.sum()) / len(st)
    assert meets_floors(n, len(st)), (case.name, level, n, share)
    bad = st & (np.asarray(got, np.int64) != np.asarray(expected, np.int64))
    return int(bad.sum()), n, share


# ---- the reference-pinned oracle paths that set the levels (key -> rows renderer); R they are compared at
PERTURB_KEYS = ("m24_po", "m24_bla", "m24_lav2_cpu", "m24_lav2_gpustage", "m53_po", "m53_bla", "m53_lav2_cpu",
                "m53_lav2_gpustage")
DIRECT_KEYS = ("m24_direct", "m53_direct", "m53_direct_hdr")


def pinned_paths(v, cap, keys):
    """{key: render_rows(y0, y1)} over the CPU oracle functions that the reference's CRC-64 goldens hold (tests/test_oracle_pins.py):
    m24 = HDRFloat<float>, m53 = HDRFloat<double>; po = CalcCpuPerturbationFractalBLA without a table, bla = with it, lav2 =
    CalcCpuPerturbationFractalLAV2 in the CPU's and the GPU's stage-test direction (_rc: over a SimpleCompression orbit); direct = CalcCpuHDR (double, HDRFloat)."""
    import _oracle
    from fractalshark_amd import inputs
    cache = {}

    _oracle.lib()  # built and loaded once, here: not by the first of several threads

    def orbit(is64, rc=False):
        if (is64, rc) not in cache:
            o = cache[(is64, rc)] = inputs.Orbit(v, is64=is64, compression_exp=20 if rc else None)
            # The library packs the orbit on the first call that asks for it (resize, then fill); a second thread arriving in
            # between would render against a half-filled orbit.  Ask for it now, on this thread.
            assert o.data_ptr
        return cache[(is64, rc)]

    def table(kind, is64, o=None):
        key = (kind, is64, id(o))
        if key not in cache:
            t = cache[key] = (inputs.LATable if kind == "la" else inputs.BLATable)(orbit(is64) if o is None else o)
            if kind == "la":
                assert t.las_ptr and t.stages_ptr
            elif t.num_levels:
                assert t.level_ptrs and t.level_sizes
        return cache[key]

    out = {}
    for key in keys:  # every input is built AND materialised here (orbit(), table()), before any renderer runs on several threads
        is64 = key.startswith("m53")
        if key.endswith("_po"):
            out[key] = lambda y0, y1, o=orbit(is64): _oracle.bla_hdr32(v, o, None, rows=(y0, y1), threads=1, n_iterations=cap)
        elif key.endswith("_bla"):
            out[key] = lambda y0, y1, o=orbit(is64), t=table("bla", is64): _oracle.bla_hdr32(
                v, o, t, rows=(y0, y1), threads=1, n_iterations=cap)
        elif key.endswith("_lav2_cpu_rc"):  # the SimpleCompression chain (Cpu32 / Cpu64 PerturbedRCBLAV2HDR): its own table
            o = orbit(is64, rc=True)
            out[key] = lambda y0, y1, o=o, t=table("la", is64, o): _oracle.lav2_hdr32(v, o, t, rows=(y0, y1), threads=1, stage_test=0,
                                                                                       n_iterations=cap)
        elif "_lav2_" in key:
            out[key] = lambda y0, y1, o=orbit(is64), t=table("la", is64), st=0 if key.endswith("_cpu") else 1: _oracle.lav2_hdr32(
                v, o, t, rows=(y0, y1), threads=1, stage_test=st, n_iterations=cap)
        elif key == "m53_direct":
            out[key] = lambda y0, y1: _oracle.direct_f64(v, rows=(y0, y1), threads=1, n_iterations=cap)
        elif key in ("m24_direct", "m53_direct_hdr"):
            out[key] = lambda y0, y1, is64=is64: _oracle.direct_hdr(v, is64, rows=(y0, y1), threads=1, n_iterations=cap)
        else:
            raise KeyError(key)
    return out


def choose_level(ladder, E, stable, got, expected):
    """The finest level of the ladder at which `got` equals `expected` on every stable, uncapped sample (E != 0), or None;
    and the misses per level."""
    per = {}
    best = None
    for j, lv in enumerate(ladder):
        st = stable[:, j] & (E != 0)
        per[str(lv)] = [int((st & (got != expected)).sum()), int(st.sum())]
        if per[str(lv)][0] == 0:
            best = lv
    return best, per


def offsets(case, got, expected, R, level):
    """Histogram {offset: samples} of got - expected over the samples stable at `level` (a recorded characterisation, for the
    paths whose reference algorithm is not an exact-count algorithm); the floors on the stable set hold here too."""
    st = case.stable(R, level)
    assert meets_floors(int(st.sum()), len(st)), (case.name, level)
    vals, cnt = np.unique((np.asarray(got, np.int64) - expected)[st], return_counts=True)
    return {str(int(a)): int(b) for a, b in zip(vals, cnt)}


def scaled_offsets(case, v, which, level, render=None):
    """Histogram {offset: samples} of a scaled kernel's output minus min(E_256 - 1, N) over the samples stable at `level`:
    the recorded characterisation of mandel_1x_float_perturb_scaled (which = "hdr32" | "f64").  render = the frame to use
    instead of the restatement's."""
    if render is None:
        import _oracle
        from fractalshark_amd import inputs
        if which == "hdr32":
            render = _oracle.gpu_scaled_hdr32(v, inputs.Orbit(v), n_iterations=case.cap)
        else:
            render = _oracle.gpu_scaled_f64(v, inputs.OrbitF64(v), n_iterations=case.cap)
    return offsets(case, case.sample(render), expect_minus_one(case.counts(256), case.cap), 256, level)
