"""A plain model of what an orbit's upload leaves on the device for the tuned loops: the prepared orbit, the two companions, the compact
zs2 / zqb of the 16-step body, the NDZ bounds znz (k_prepare_orbit_hdr32 / _hdr64, k_make_quiet_orbit in csrc/kernels_orbit_prep.hip,
k_decompress_orbit_hdr32 in csrc/kernels_decompress.hip) and the scaled kernels' bound word (k_scaled_bounds in csrc/kernels_scaled.hip) -- numpy only, nothing of the product
imported, written from the DEFINITIONS in the comments there and in csrc/scaled_runs.hpp:

  prepared     {re, im, e, 2^(8 - 2 max(e, -1000))}: hc_from_hr of the entry (tests/_ieee_model.py), .w = +inf where it overflows;
               HDRFloat<double>: the clamp at -500.  The two spare entries are zero words.
  first        {re, im, ~e + 116 for e <= 2 else 1 << 24, 0}
  own bound    zmax = max part 2^clamp(e, -200, 100);  zmax / 4 where 2^-40 <= zmax < 5.6 and min part >= max part 2^-40, else "never"
               (the bit pattern 0x80000000)
  block bound  the smallest own[j + k + 1] / (g_j .. g_(j+k)), k = 0 .. 3, g = (4 zmax + 3.8)(1 + 2^-10), times (1 - 2^-10); "never" with a
               zmax >= 5.6 among j .. j + 3, an arrival without a bound, or j past the end; reads past the end see the last entry
  second       {2Z.re, 2Z.im, own, block}, 2Z = part 2^(e + 1);   zs2 = its .xy;   zqb[i] = block bounds of i + 3, i + 7, i + 11, i + 15
  znz          the two NDZ body bounds as the comment of ndz_body_bound defines them
  slack        32 entries behind zs2 / zqb (zero words) and znz ("never")
  scaled word  M / 4, M = max(|x|, |y|), or -1.0 for a `bad` entry, the last entry, or M outside [2^-40, 5.6)

Every operation is ONE binary32 operation (the library is built with -ffp-contract=off; *, /, +, fmin are IEEE operations and ldexp
by a power of two is one rounding), so numpy's float32 arithmetic is the model; tests/test_gpu_quiet_orbit.py holds the device to it bit
for bit.  tests/test_quiet_model_cpu.py holds the model to what the bounds are FOR (check_blocks, check_bodies16, check_own_purpose,
check_scaled_purpose below) and shows that three mutants of it (the keyword arguments of Tables) fail there."""
import functools
from fractions import Fraction

import numpy as np

import _ieee_model as im

F = np.float32
NEVER = 0x80000000
SLACK = 32
_NEVER_F = np.array([NEVER], np.uint32).view(np.float32)[0]
_C56, _K10U, _K10D = F(5.6), F(1.0) + F(2.0 ** -10), F(1.0) - F(2.0 ** -10)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def is_never(a):
    return bits(a) == NEVER


def ldexp32(x, k):
    """x 2^k rounded once to binary32 (x float32, k integers of any size)"""
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(np.asarray(x, np.float64), np.clip(np.asarray(k, np.int64), -4000, 4000).astype(np.int32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _from_hr(T, mx, ex, my, ey):
    return im.hc_from_hr(T, (mx, ex), (my, ey))


def prepared(entries):
    """the prepared HDRFloat<float> orbit of entries() -> (count + 2, 4) float32 (.z holds the exponent's bits)"""
    n = len(entries)
    out = np.zeros((n + 2, 4), np.float32)
    e = np.zeros(n, np.int32)
    for i, (mx, ex, ey, my) in enumerate(entries.tolist()):
        out[i, 0], out[i, 1], e[i] = _from_hr(im.R32, mx, ex, my, ey)
    out[:n, 2] = e.view(np.float32)
    with np.errstate(over="ignore"):
        out[:n, 3] = np.ldexp(1.0, 8 - 2 * np.maximum(e, -1000)).astype(np.float32)
    return out


PREPARED64 = np.dtype([("re", "<f8"), ("im", "<f8"), ("e", "<i4"), ("pad", "<i4"), ("w", "<f8")])


def prepared64(entries):
    n = len(entries)
    out = np.zeros(n + 2, PREPARED64)
    for i, (mx, ex, _, ey, _, my) in enumerate(entries.tolist()):
        out["re"][i], out["im"][i], out["e"][i] = _from_hr(im.R64, mx, ex, my, ey)
    out["w"][:n] = np.ldexp(1.0, 8 - 2 * np.maximum(out["e"][:n], -500))
    return out


class Tables:
    """Everything k_make_quiet_orbit derives from a prepared orbit (n, 4).  The keyword arguments are the mutants of the teeth test."""

    def __init__(self, prep, growth=3.8, arrival_shift=1, zqb_offsets=(3, 7, 11, 15)):
        with np.errstate(all="ignore"):
            self._make(np.ascontiguousarray(prep, np.float32), F(growth), arrival_shift, zqb_offsets)

    def _make(self, prep, growth, shift, offsets):
        n = prep.shape[0]
        self.n, self.prepared = n, prep
        x, y = prep[:, 0], prep[:, 1]
        e = np.ascontiguousarray(prep[:, 2]).view(np.int32)
        self.first = np.zeros((n, 4), np.float32)
        self.first[:, 0], self.first[:, 1] = x, y
        self.first[:, 2] = np.where(e <= 2, ~e + 116, 1 << 24).astype(np.int32).view(np.float32)
        # own bound
        hi, lo = np.maximum(np.abs(x), np.abs(y)), np.minimum(np.abs(x), np.abs(y))
        zmax = ldexp32(hi, np.clip(e, -200, 100))
        usable = (zmax >= F(2.0 ** -40)) & (zmax < _C56) & (lo >= hi * F(2.0 ** -40))
        self.zmax = zmax
        self.own = np.where(usable, zmax * F(0.25), _NEVER_F).astype(np.float32)
        # block bound of j = 0 .. n + 15 (never past the end)
        jj = np.arange(n + 16)
        best, grow, ok = np.full(n + 16, F(2.0 ** 60)), np.full(n + 16, F(1.0)), jj < n
        for k in range(4):
            m = zmax[np.minimum(jj + k, n - 1)]
            ok &= m < _C56
            grow = grow * ((F(4.0) * m + growth) * _K10U)
            a = jj + k + shift
            bk = np.where(a < n, self.own[np.minimum(a, n - 1)], _NEVER_F).astype(np.float32)
            ok &= ~is_never(bk)
            best = np.fmin(best, bk / grow)
        blk = np.where(ok, best * _K10D, _NEVER_F).astype(np.float32)
        self.block = blk[:n]
        z2x, z2y = ldexp32(x, e.astype(np.int64) + 1), ldexp32(y, e.astype(np.int64) + 1)
        self.second = np.stack([z2x, z2y, self.own, self.block], axis=1)
        self.zs2 = np.zeros((n + SLACK, 2), np.float32)
        self.zs2[:n, 0], self.zs2[:n, 1] = z2x, z2y
        self.zqb = np.zeros((n + SLACK, 4), np.float32)
        for c, off in enumerate(offsets):
            self.zqb[:n, c] = blk[np.arange(n) + off]
        # NDZ body bounds
        j = np.arange(n)
        zr, zi = np.abs(np.concatenate([z2x, np.zeros(8, np.float32)])), np.abs(np.concatenate([z2y, np.zeros(8, np.float32)]))
        ok = (j + 8 < n) & ~is_never(blk[j]) & ~is_never(blk[j + 4])
        bd, bc, a, b = (np.full(n, F(v)) for v in (2.0 ** 60, 2.0 ** 60, 1.0, 0.0))
        for m in range(8):
            lo = np.fmin(zr[j + m], zi[j + m])
            ok &= lo >= F(2.0 ** -100)
            bd = np.fmin(bd, lo * F(2.0 ** -27) / a)
            if m:
                bc = np.fmin(bc, lo * F(2.0 ** -27) / b)
            s = (zr[j + m] + zi[j + m]) * _K10U
            b = s * b + F(1.0)
            a = a * s
        sb = np.concatenate([self.own, np.zeros(8, np.float32)])[j + 8] * F(0.5)
        bd = np.fmin(bd, sb / a) * _K10D
        bc = np.fmin(bc, sb / b) * _K10D
        ok &= (bd >= F(2.0 ** -120)) & (bd < F(2.0 ** 60)) & (bc >= F(2.0 ** -120)) & (bc < F(2.0 ** 60))
        self.znz = np.full((n + SLACK, 2), _NEVER_F, np.float32)
        self.znz[:n, 0], self.znz[:n, 1] = np.where(ok, bd, _NEVER_F), np.where(ok, bc, _NEVER_F)

    def parts(self):
        return {"prepared": self.prepared, "first": self.first, "second": self.second, "zs2": self.zs2, "zqb": self.zqb, "znz": self.znz}

    def counts(self):
        return counts(self.parts())


def counts(parts):
    """entries with an own bound, with a block bound, with NDZ bounds -- of a model's parts or of a read-back"""
    return {"own": int((~is_never(parts["second"][:, 2])).sum()), "block": int((~is_never(parts["second"][:, 3])).sum()),
            "ndz": int((~is_never(parts["znz"][:, 0])).sum())}


SCALED = np.dtype([("bad", "<u4"), ("padding", "<u4"), ("x", "<f4"), ("y", "<f4")])


def scaled_words(ent):
    """the bound word of every binary32 entry (SCALED records) as a bit pattern"""
    n = len(ent)
    m = np.fmax(np.abs(ent["x"]), np.abs(ent["y"]))
    usable = (ent["bad"] == 0) & (np.arange(n) + 1 < n) & (m >= F(2.0 ** -40)) & (m < _C56)
    return bits(np.where(usable, m * F(0.25), F(-1.0)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ what the bounds are for
def start_states(rng):
    """Rows of (dz.re, dz.im, dc.re, dc.im) in units of the bound on max|dz| (the first two) and on max|dc| (the last two): both parts of dz at +-1 and at +-2^-k against +-1, dc at +-1, all
    sign combinations; then seeded random states within the bound."""
    rows = []
    signs = [(a, b, c, d) for a in (1, -1) for b in (1, -1) for c in (1, -1) for d in (1, -1)]
    for k in (0, 1, 12, 30):
        for big_re in ((True,) if k == 0 else (True, False)):
            x, y = (1.0, 2.0 ** -k) if big_re else (2.0 ** -k, 1.0)
            rows += [(a * x, b * y, c * 1.0, d * 1.0) for a, b, c, d in signs]
    rows += [tuple(rng.uniform(-1.0, 1.0, 4)) for _ in range(24)]
    # (and dc far below dz, the case the add-free runs are in)
    rows += [(a, b, c * 2.0 ** -40, d * 2.0 ** -40) for a, b, c, d in signs[:8]]
    return np.array(rows, np.float64)


def on_the_bound(st):
    """every row scaled so that its largest component is exactly 1"""
    return st / np.abs(st).max(axis=1, keepdims=True)


class _Run:
    """States (entries j) x (rows of `st`) started with max(max|dz|, max|dc|) = g[j] st, in a run's scale: w = dz 2^-E with max|w| near
    2^-24 (E a power of two: scaling changes no bit), stepped as the full form steps, each operation rounded once."""

    def __init__(self, second, j, g, st):
        self.t, self.j, self.k = second, j, 0
        g = g.astype(np.float64)[:, None]
        E = np.floor(np.log2(g)) + 24.0
        self.sc, isc = np.exp2(E), np.exp2(-E)
        self.w_re, self.w_im = (st[None, :, 0] * g * isc).astype(np.float32), (st[None, :, 1] * g * isc).astype(np.float32)
        self.dc_re, self.dc_im = (st[None, :, 2] * g * isc).astype(np.float32), (st[None, :, 3] * g * isc).astype(np.float32)
        # (rounding a state to binary32 must not carry it over the bound)
        assert (self.G() <= g).all()

    def max_dz(self):
        return np.maximum(np.abs(self.w_re), np.abs(self.w_im)).astype(np.float64) * self.sc

    def G(self):
        return np.maximum(self.max_dz(), np.maximum(np.abs(self.dc_re), np.abs(self.dc_im)).astype(np.float64) * self.sc)

    def dz(self):
        return self.w_re.astype(np.float64) * self.sc, self.w_im.astype(np.float64) * self.sc

    def step(self):
        """one step from entry j + k to entry j + k + 1; -> the index of the entry arrived at"""
        at = np.minimum(self.j + self.k, self.t.shape[0] - 1)
        z_re, z_im = self.t[at, 0][:, None].astype(np.float64), self.t[at, 1][:, None].astype(np.float64)
        # s = fma(w, 2^E, 2Z): evaluated in binary64, rounded to binary32 once
        s_re = (self.w_re.astype(np.float64) * self.sc + z_re).astype(np.float32)
        s_im = (self.w_im.astype(np.float64) * self.sc + z_im).astype(np.float32)
        # p = w s (two products and a sum per part), q = p + dc 2^-E
        p_re = (self.w_re * s_re) - (self.w_im * s_im)
        p_im = (self.w_re * s_im) + (self.w_im * s_re)
        self.w_re, self.w_im = p_re + self.dc_re, p_im + self.dc_im
        assert self.w_re.dtype == np.float32 and self.w_im.dtype == np.float32
        self.k += 1
        return self.j + self.k


def _own_at(t, idx):
    """own bound of the entries idx as float64, -1 ("nothing passes") for "never" and past the end"""
    n = t.shape[0]
    own = t[np.minimum(idx, n - 1), 2]
    return np.where((idx < n) & ~is_never(own), own.astype(np.float64), -1.0)[:, None]


def check_blocks(second, guard, offset, st, purpose=None):
    """The definition of a block bound: a state at entry j + offset with max(max|dz|, max|dc|) ON guard[j] (the word that licenses the
    block starting there) takes four steps, and each arrival's max|dz| is within the own bound of the entry it arrives at.
    -> (blocks started, violations [(j, row, step)]).  purpose: called with (second, entry indices, dz.re, dz.im) per arrival."""
    with np.errstate(all="ignore"):
        j = np.nonzero(~is_never(guard) & (np.arange(len(guard)) + offset < second.shape[0]))[0]
        if j.size == 0:
            return 0, []
        run = _Run(second, j + offset, guard[j], st)
        bad = []
        for k in range(4):
            at = run.step()
            ok = run.max_dz() <= _own_at(second, at)
            bad += [(int(j[a]), int(c), k) for a, c in zip(*np.nonzero(~ok))]
            if purpose is not None and not bad:
                purpose(second, at, *run.dz())
        return int(j.size), bad


def check_zqb(second, zqb, st, offsets=(3, 7, 11, 15)):
    """zqb[i]'s words license the blocks that start at the entries i + 3, i + 7, i + 11, i + 15: check_blocks for each word.  A column
    that IS the second companion's .w at its offset, bit for bit ("never" past the end), names the pairs (entry, bound) check_blocks
    has been through with .w itself and is not stepped again.  -> (columns stepped, violations)"""
    n = second.shape[0]
    blk = np.concatenate([bits(second[:, 3]), np.full(16, NEVER, np.uint32)])
    stepped, bad = 0, []
    for c, off in enumerate(offsets):
        if np.array_equal(bits(zqb[:n, c]), blk[np.arange(n) + off]):
            continue
        stepped += 1
        bad += [(c,) + v for v in check_blocks(second, zqb[:n, c], off, st)[1]]
    return stepped, bad


def check_bodies16(second, zqb, st, scales=(0, -12, -24)):
    """The 16-step body (FS_FAST_LOOP_FD16P): a body that starts with the state at entry j (first arrival i = j + 1) reads zqb[i]; its
    blocks are licensed by the block bound of j itself (the second companion's .w: the caller's, or .w of the record before), then by
    zqb[i].x / .y / .z against the states after 4 / 8 / 12 steps.  Wherever all four tests pass, all sixteen arrivals pass their own
    tests.  Started on the first bound and 2^scales below it (a state ON the first bound has usually outgrown the second).
    -> (bodies x rows whose four tests all pass, violations)."""
    n = second.shape[0]
    with np.errstate(all="ignore"):
        j = np.nonzero(~is_never(second[:, 3]))[0]
        j = j[j + 1 < n]
        passed, bad = 0, []
        for sc in scales:
            if j.size == 0:
                break
            run = _Run(second, j, second[j, 3] * F(2.0 ** sc), st)
            alive = np.ones((j.size, st.shape[0]), bool)
            arrivals_ok = np.ones_like(alive)
            for k in range(16):
                if k in (4, 8, 12):
                    word = zqb[j + 1, k // 4 - 1]
                    alive &= run.G() <= np.where(is_never(word), -1.0, word.astype(np.float64))[:, None]
                at = run.step()
                arrivals_ok &= ~alive | (run.max_dz() <= _own_at(second, at))
            passed += int(alive.sum())
            bad += [(int(j[a]), int(c), sc) for a, c in zip(*np.nonzero(alive & ~arrivals_ok))]
        return passed, bad


def _frac(v):
    return Fraction(float(v))


def _exactly(zx, zy, ux, uy, ratio, cap):
    zx, zy, ux, uy = _frac(zx), _frac(zy), _frac(ux), _frac(uy)
    z2, d2 = (zx + ux) ** 2 + (zy + uy) ** 2, ux * ux + uy * uy
    return z2 >= ratio * d2 and z2 < cap


def purpose_violations(zx, zy, ux, uy, ratio, cap):
    """|Z + dz|^2 >= ratio |dz|^2 and |Z + dz|^2 < cap, decided exactly for every element (float64 arrays of exact values; ratio a
    Fraction).  A binary64 evaluation decides where its error bound (2^-48 of the terms' absolute sum, a hundred times what eight
    roundings can lose) leaves no doubt; everything else goes through fractions.Fraction.  -> (indices that violate, elements decided
    by Fraction)."""
    r = float(ratio)
    lhs = zx * zx + zy * zy + 2.0 * (zx * ux + zy * uy) + (1.0 - r) * (ux * ux + uy * uy)
    mag = zx * zx + zy * zy + 2.0 * (np.abs(zx * ux) + np.abs(zy * uy)) + (1.0 + r) * (ux * ux + uy * uy)
    z2 = (zx + ux) ** 2 + (zy + uy) ** 2
    sure = (lhs > mag * 2.0 ** -48) & (z2 * (1.0 + 2.0 ** -48) < cap) & np.isfinite(mag)
    doubt = np.nonzero(~sure)
    bad = [tuple(int(x) for x in ix) for ix in zip(*doubt)
           if not _exactly(zx[ix], zy[ix], ux[ix], uy[ix], ratio, cap)]
    return bad, len(doubt[0])


def own_purpose(second, at, ux, uy):
    """what the own bound is for (csrc/kernels_lav2_hdr32.hip, the scaled runs): an arrival within it neither rebases nor escapes"""
    zx, zy = (second[at, c].astype(np.float64)[:, None] * 0.5 + 0.0 * ux for c in (0, 1))
    bad, exact = purpose_violations(zx, zy, ux, uy, Fraction(1), 256)
    assert not bad, ("an arrival within its own bound would rebase or escape", [(int(at[a]), c) for a, c in bad[:6]])
    own_purpose.decided_exactly += exact
    own_purpose.arrivals += ux.size


own_purpose.decided_exactly = own_purpose.arrivals = 0


def check_own_purpose(second, st):
    """... and for arrivals ON the own bound: dz with its larger part exactly on it, every row of st"""
    j = np.nonzero(~is_never(second[:, 2]))[0]
    g = second[j, 2].astype(np.float64)[:, None]
    d = on_the_bound(st[:, :2])
    own_purpose(second, j, g * d[None, :, 0], g * d[None, :, 1])
    return int(j.size)


def check_scaled_purpose(ent, words, st):
    """the scaled kernels' M / 4: |z|^2 >= 3.3 |dz|^2 and |z|^2 < 115 for every dz with max part <= the word, tried ON it"""
    # (fmax passes over a NaN part -- no orbit has one -- and the word is then made of the other part: held bit for bit, nothing to claim)
    j = np.nonzero((words != bits(np.array([-1.0], np.float32))[0]) & np.isfinite(ent["x"]) & np.isfinite(ent["y"]))[0]
    g = words[j].view(np.float32).astype(np.float64)[:, None]
    d = on_the_bound(st[:, :2])
    zx, zy = (ent[c][j].astype(np.float64)[:, None] + 0.0 * g * d[None, :, 0] for c in ("x", "y"))
    bad, _ = purpose_violations(zx, zy, g * d[None, :, 0], g * d[None, :, 1], Fraction(33, 10), 115)
    return int(j.size), [(int(j[a]), c) for a, c in bad]
