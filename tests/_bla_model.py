"""A plain model of the BLA lookup and of the tables the device derives from a BLA table (test infrastructure).

Inputs are the host builder's level arrays (inputs.BLATable.level), m_LM2 and the orbit's entries; nothing here follows the
loop structure of a kernel.  Three things are modelled:

  lookup_backwards   BLAS::LookupBackwards (BLAS.cpp:256-310), read straight off the reference: the answer every device lookup
                     must give.  A value is the pair (exponent, mantissa); "z2 < r2" is the reduced-positive compare of
                     HDRFloat.h:1150-1167 -- exponent first, then mantissa -- which is Python's tuple compare of such pairs.
  native / heap      the derived tables of an HDRFloat<float> table, each element from its definition (kernels.h FsBlaRec and
                     ladder, k_bla_make_kmax's pre-test keys; kernels_bla_fast.hip: heap records, heap ladder, Q, zb), as numpy
                     arrays whose bytes are the device's.
  walk_native /      the lookup as the header comments of kernels_perturb.hip / kernels_bla_fast.hip describe it over those
  walk_heap          tables (pre-test, first round from the Q entry's four keys, later rounds from the heap ladder at sixteen
                     times the position), so that tables read back from a device can be asked the whole question set.
"""
import numpy as np

from fractalshark_amd import inputs

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
K_POISON_EXP = -(1 << 28)       # kPoisonExp: arrival exponent of a record / entry the fast forms must not use
K_POISON_EXP_HIGH = 1 << 27     # kPoisonExpHigh: true-exponent slot of an entry no step may arrive at
FIRST_LEVEL = 2                 # BLAS.h:22
MIN_BIG_EXP = -268435456        # HDRFloat's MIN_BIG_EXPONENT: the exponent of its zero

BLA_HDR64_DTYPE = np.dtype([("r2_m", "<f8"), ("r2_e", "<i4"), ("p0", "<i4"), ("Ax_m", "<f8"), ("Ax_e", "<i4"), ("p1", "<i4"),
                            ("Ay_m", "<f8"), ("Ay_e", "<i4"), ("p2", "<i4"), ("Bx_m", "<f8"), ("Bx_e", "<i4"), ("p3", "<i4"),
                            ("By_m", "<f8"), ("By_e", "<i4"), ("p4", "<i4"), ("l", "<i4"), ("p5", "<i4")])
assert BLA_HDR64_DTYPE.itemsize == 88
REC_DTYPE = np.dtype([("Axm", "<f4"), ("Aym", "<f4"), ("Bxm", "<f4"), ("Bym", "<f4"), ("Axe", "<i4"), ("Aye", "<i4"),
                      ("Bxe", "<i4"), ("Bye", "<i4"), ("Zre", "<f4"), ("Zim", "<f4"), ("Ze", "<i4"), ("l", "<u4")])
assert REC_DTYPE.itemsize == 48
Q_DTYPE = np.dtype([("key", "<i8"), ("pos", "<u4"), ("lvl", "<i4"), ("k", "<i8", (4,))])
assert Q_DTYPE.itemsize == 48
ZB_DTYPE = np.dtype([("re", "<f4"), ("im", "<f4"), ("e", "<i4"), ("quiet", "<i4")])


# ---------------------------------------------------------------------------------------------- the reference's lookup
def lookup_backwards(levels, lm2, m, z2):
    """BLAS::LookupBackwards.  levels[L][ix] = r2 of element ix of level L as (exponent, mantissa); z2 likewise.
    -> (level, index) or None."""
    if m == 0:
        return None
    k = m - 1
    if (k & 1) == 1:
        return None
    if k == 0:
        if not z2 < levels[FIRST_LEVEL][0]:
            return None
        zeros = 32
        ix = 0
    else:
        zeros = (k & -k).bit_length() - 1  # the exponent of (float)(k & -k)
        ix = k >> zeros                    # (from zeros, not from the capped level)
    level = zeros if zeros <= lm2 else lm2
    while level >= FIRST_LEVEL:
        if z2 < levels[level][ix]:
            return (level, ix)
        ix <<= 1
        level -= 1
    return None


def probes(lm2, m):
    """The (level, index) pairs the walk of lookup_backwards probes at m, in its order; [] where there is no walk (m = 0, an
    odd k, a start level below 2).  The gate of k = 0 is not part of the list."""
    if m == 0 or ((m - 1) & 1):
        return []
    k = m - 1
    zeros = 32 if k == 0 else (k & -k).bit_length() - 1
    ix = 0 if k == 0 else k >> zeros
    out = []
    for level in range(min(zeros, lm2), FIRST_LEVEL - 1, -1):
        out.append((level, ix))
        ix <<= 1
    return out


# ---------------------------------------------------------------------------------------------- tables and questions
class Table:
    """The host builder's table as the model reads it."""

    def __init__(self, bla):
        self.is64 = bool(bla.is64)
        self.lm2 = int(bla.lm2)
        self.n_levels = int(bla.num_levels)
        self.sizes = [int(x) for x in bla.sizes()]
        dt = BLA_HDR64_DTYPE if self.is64 else inputs.BLA_HDR32_DTYPE
        self.raw = [bla.level(l) for l in range(self.n_levels)]
        self.rec = [a.view(dt).reshape(-1) for a in self.raw]
        self.r2 = [list(zip(a["r2_e"].tolist(), a["r2_m"].tolist())) for a in self.rec]

    def lookup(self, m, z2):
        return lookup_backwards(self.r2, self.lm2, m, z2)


def _neighbours(e, mant, is64):
    """The value, and the values whose mantissa bit pattern is one below / above, where that is still a positive finite float."""
    ft, it = (np.float64, np.int64) if is64 else (np.float32, np.int32)
    inf_bits = int(np.array(np.inf, ft).view(it))
    bits = int(np.array(mant, ft).view(it))
    out = []
    for d in (-1, 0, 1):
        b = bits + d
        if 0 <= b < inf_bits:
            out.append((e, float(np.array(b, it).view(ft))))
    return out


def question_set(tab, count):
    """Every m of the orbit x {below, at, above the r2 of every record the walk (and the gate of m = 1) probes; zero; the
    HDRFloat zero; the largest finite value} -> list of (m, (exponent, mantissa))."""
    fmax = float(np.finfo(np.float64 if tab.is64 else np.float32).max)
    fixed = [(0, 0.0), (MIN_BIG_EXP, 0.0), (0x7FFFFFFF, fmax)]
    out = []
    for m in range(count):
        keys = list(fixed)
        pr = probes(tab.lm2, m)
        if m == 1:
            pr = [(FIRST_LEVEL, 0)] + pr
        for (L, ix) in pr:
            e, mant = tab.r2[L][ix]
            keys += _neighbours(e, mant, tab.is64)
        out += [(m, z) for z in keys]
    return out


def pack_questions(qs, is64):
    """-> (m uint32[n], z2 REAL_HDR32 / REAL_HDR64 [n]) for the oracle export and the device probe."""
    m = np.array([q[0] for q in qs], np.uint32)
    z2 = np.zeros(len(qs), inputs.REAL_HDR64 if is64 else inputs.REAL_HDR32)
    z2["m"] = [q[1][1] for q in qs]
    z2["e"] = np.array([q[1][0] for q in qs], np.int64).astype(np.int32)
    return m, z2


def answers(tab, qs):
    """The model's answers in the probes' output form: uint32[n, 2], 0xFFFFFFFF twice for none."""
    out = np.full((len(qs), 2), 0xFFFFFFFF, np.uint32)
    for i, (m, z) in enumerate(qs):
        a = tab.lookup(m, z)
        if a is not None:
            out[i] = a
    return out


CLASSES = ("m0", "k0_gate_open", "k0_gate_shut", "odd_k", "start_below_2", "hit_probe_1", "hit_probe_2", "hit_probe_3",
           "hit_probe_4", "hit_round_2", "hit_round_3", "miss_pretest_rejects", "miss_passes_pretest")


def classify(tab, m, z2):
    """The classes a question falls into (the gate classes of k = 0 come on top of the walk's outcome)."""
    if m == 0:
        return ["m0"]
    k = m - 1
    if k & 1:
        return ["odd_k"]
    out = []
    if k == 0:
        if not z2 < tab.r2[FIRST_LEVEL][0]:
            return ["k0_gate_shut"]
        out.append("k0_gate_open")
    pr = probes(tab.lm2, m)
    if not pr:
        return out + ["start_below_2"]
    for n, (L, ix) in enumerate(pr):
        if z2 < tab.r2[L][ix]:
            return out + [("hit_probe_%d" % (n + 1)) if n < 4 else ("hit_round_%d" % (n // 4 + 1))]
    # nothing holds: the pre-test key is the largest r2 the walk meets
    return out + ["miss_pretest_rejects" if not z2 < max(tab.r2[L][ix] for (L, ix) in pr) else "miss_passes_pretest"]


# ---------------------------------------------------------------------------------------------- the derived tables (float)
def key_of(e, mant):
    """exponent << 32 | mantissa bits, as a signed 64-bit number (one integer compare = the reduced-positive compare)."""
    bits = int(np.array(mant, np.float32).view(np.uint32))
    v = ((int(e) & 0xFFFFFFFF) << 32) | bits
    return v - (1 << 64) if v >> 63 else v


def prepared_orbit(entries):
    """The orbit as the kernels hold it, HDRFloatComplex from two HDRFloat (HDRFloatComplex.h:166-173): the larger exponent, each
    mantissa times getMultiplier(its exponent - that one) (0 at -127 and below).  -> (re f4, im f4, e i4)."""
    ex, ey = entries["ex"].astype(np.int64), entries["ey"].astype(np.int64)
    e = np.maximum(ex, ey)

    def mult(s):
        return np.where(s <= -127, np.float32(0), np.ldexp(np.float32(1), np.maximum(s, -126).astype(np.int32))).astype(np.float32)
    with np.errstate(all="ignore"):
        re = (entries["mx"] * mult(ex - e)).astype(np.float32)
        im = (entries["my"] * mult(ey - e)).astype(np.float32)
    return re, im, e.astype(np.int32)


def heap_height(level_n):
    """H = the largest L + ceil(log2(elements of L)); 0 = no heap (below 3, or positions of 2^24 and more)."""
    H = 0
    for L in range(FIRST_LEVEL, min(len(level_n), 40)):
        if level_n[L]:
            H = max(H, L + (level_n[L] - 1).bit_length())
    return 0 if (H < 3 or H - 1 > 24) else H


class Derived:
    """Everything the device derives from (table, orbit), HDRFloat<float>."""

    def __init__(self, tab, entries):
        assert not tab.is64 and tab.n_levels > FIRST_LEVEL
        self.tab = tab
        self.count = count = len(entries)
        self.zre, self.zim, self.ze = prepared_orbit(entries)
        nl = tab.n_levels
        self.level_n = [0, 0] + tab.sizes[2:]
        self.level_off = [0] * nl
        total = 0
        for L in range(FIRST_LEVEL, nl):
            self.level_off[L] = total
            total += self.level_n[L]
        self.total = total
        self.n_q = count // 4 + 2
        # keys of every record; one that is negative or not finite makes the integer compare differ: no native form then
        self.keys = [np.zeros(0, np.int64)] * nl
        self.bad = False
        for L in range(FIRST_LEVEL, nl):
            bits = tab.rec[L]["r2_m"].view(np.int32).astype(np.int64)
            self.bad |= bool(np.any((bits < 0) | ((bits & 0x7F800000) == 0x7F800000)))
            self.keys[L] = (tab.rec[L]["r2_e"].astype(np.int64) << 32) | bits
        # ---- native records and ladder
        self.records = np.zeros(total, REC_DTYPE)
        self.ladder = np.full((total, 4), INT64_MIN, np.int64)
        self.arrive = np.zeros(total, np.int64)
        self.level_of = np.zeros(total, np.int32)
        self.ix_of = np.zeros(total, np.int64)
        for L in range(FIRST_LEVEL, nl):
            n, o = self.level_n[L], self.level_off[L]
            src, dst = tab.rec[L], self.records[o:o + n]
            ix = np.arange(n, dtype=np.int64)
            for a, b in (("Axm", "Ax_m"), ("Aym", "Ay_m"), ("Bxm", "Bx_m"), ("Bym", "By_m"), ("Axe", "Ax_e"), ("Aye", "Ay_e"),
                         ("Bxe", "Bx_e"), ("Bye", "By_e")):
                dst[a] = src[b]
            dst["l"] = src["l"].view(np.uint32)
            arrive = (ix << L) + 1 + dst["l"].astype(np.int64)
            inside = arrive < count
            at = np.where(inside, arrive, 0)
            dst["Zre"] = np.where(inside, self.zre[at], np.float32(0))
            dst["Zim"] = np.where(inside, self.zim[at], np.float32(0))
            dst["Ze"] = np.where(inside, self.ze[at], 0)
            self.arrive[o:o + n], self.level_of[o:o + n], self.ix_of[o:o + n] = arrive, L, ix
            for j in range(4):
                if L - j >= FIRST_LEVEL:
                    self.ladder[o:o + n, j] = self.keys[L - j][ix << j]
        # ---- pre-test keys
        self.pretest = np.zeros(self.n_q, np.int64)
        for q in range(self.n_q):
            self.pretest[q] = self.pretest_key(q)
        # ---- heap forms
        self.H = H = heap_height(self.level_n)
        self.heap_positions = (1 << (H - 1)) if H else 0
        if not H:
            return
        hp = self.heap_positions
        self.heap_records = np.zeros(hp, REC_DTYPE)  # positions no record maps to stay zero
        self.heap_ladder = np.zeros((hp, 4), np.int64)
        h = (1 << (H - self.level_of.astype(np.int64))) + self.ix_of
        assert len(np.unique(h)) == total and h.max() < hp
        rec = self.records.copy()
        self.reasons = self.poison_reasons()
        rec["Ze"] = np.where(self.reasons["any"], K_POISON_EXP, rec["Ze"])
        rec["l"] = np.where(self.reasons["leaves"], np.uint32(0xFFFFFFFF), rec["l"])
        self.heap_records[h] = rec
        self.heap_ladder[h] = self.ladder
        self.heap_pos_of = h
        self.q = np.zeros(self.n_q, Q_DTYPE)
        for q in range(self.n_q):
            self.q[q] = self.q_entry(q)
        # ---- zb: the orbit as the steps read it, two entries beyond its end
        n = count + 2
        zb = np.zeros(n, ZB_DTYPE)
        zb["re"][:count], zb["im"][:count] = self.zre, self.zim
        e = np.zeros(n, np.int64)
        e[:count] = self.ze
        i = np.arange(n)
        arrivable = (i < count) & (e > -(1 << 26))
        quiet_ok = arrivable & (e <= 1) & (e >= -40) & (i + 1 < count)
        zb["e"] = np.where(arrivable, e, K_POISON_EXP_HIGH)
        zb["quiet"] = np.where(quiet_ok, e - 4, K_POISON_EXP)
        self.zb = zb
        self.zb_kind = np.where(quiet_ok, 0, np.where(arrivable, 1, 2))  # quiet arrival / arrival with z only / none

    def poison_reasons(self):
        """Per native position, why the quiet jump may not be taken (k_bla_make_heap's comment, rule by rule)."""
        r = self.records
        with np.errstate(all="ignore"):
            amx = np.fmax(np.fmax(np.abs(r["Axm"]), np.abs(r["Aym"])), np.fmax(np.abs(r["Bxm"]), np.abs(r["Bym"])))
        emin = np.minimum(np.minimum(r["Axe"], r["Aye"]), np.minimum(r["Bxe"], r["Bye"]))
        out = {"mantissa": ~(amx <= np.float32(2.0 ** 30)), "exponent": ~(emin > -(1 << 26)),
               "arrival_high": r["Ze"] > 1, "arrival_low": r["Ze"] < -40,
               "last_entry": self.arrive + 1 == self.count, "leaves": self.arrive >= self.count}
        out["any"] = np.zeros(len(r), bool)
        for k in ("mantissa", "exponent", "arrival_high", "arrival_low", "last_entry", "leaves"):
            out["any"] = out["any"] | out[k]
        return out

    def walk_of_q(self, q):
        """The walk at m = 4 q + 1 as positions: list of (level, index), None where it would index beyond a level."""
        pr = probes(self.tab.lm2, 4 * q + 1)
        for (L, ix) in pr:
            if L >= self.tab.n_levels or ix >= self.level_n[L]:
                return None
        return pr

    def pretest_key(self, q):
        pr = probes(self.tab.lm2, 4 * q + 1)
        if not pr:
            return INT64_MIN
        if self.walk_of_q(q) is None:
            return INT64_MAX
        return max(int(self.keys[L][ix]) for (L, ix) in pr)

    def q_entry(self, q):
        never = (INT64_MIN,) * 4
        pr = probes(self.tab.lm2, 4 * q + 1)
        if not pr:
            return (INT64_MIN, 0, 0, never)                       # no walk at this index: never passes
        if self.walk_of_q(q) is None:
            return (int(self.pretest[q]), 0, 0, never)            # the heap numbering cannot name the start: the slow lookup
        L, ix = pr[0]
        key = int(self.pretest[q])
        if q == 0:
            key = min(key, int(self.keys[FIRST_LEVEL][0]))        # the gate of BLAS.cpp:270-281
        return (key, (1 << (self.H - L)) + ix, L, tuple(int(x) for x in self.ladder[self.level_off[L] + ix]))

    # ---- bytes, in the order fs_read_bla_native hands the parts out
    def part_bytes(self):
        out = {"records": self.records.tobytes(), "ladder": self.ladder.tobytes(), "pretest": self.pretest.tobytes()}
        if self.H:
            out.update({"heap_records": self.heap_records.tobytes(), "heap_ladder": self.heap_ladder.tobytes(),
                        "q": self.q.tobytes(), "zb": self.zb.tobytes()})
        return out


# ---------------------------------------------------------------------------------------------- the lookups over those tables
def _first_below(zkey, four):
    for n in range(4):
        if zkey < int(four[n]):
            return n
    return 4


def walk_native(ladder, pretest, level_off, lm2, m, zkey):
    """The lookup on the ladder and the pre-test keys (kernels_perturb.hip, bla_lookup_native) -> native position or None."""
    if m == 0 or ((m - 1) & 1):
        return None
    k = m - 1
    zeros = 32 if k == 0 else (k & -k).bit_length() - 1
    ix = 0 if k == 0 else k >> zeros
    L = min(zeros, lm2)
    if L < FIRST_LEVEL:
        return None
    if k == 0 and not zkey < int(ladder[level_off[FIRST_LEVEL]][0]):
        return None
    if not zkey < int(pretest[k >> 2]):
        return None
    while L >= FIRST_LEVEL:
        nf = _first_below(zkey, ladder[level_off[L] + ix])
        if nf < 4:
            return level_off[L - nf] + (ix << nf)
        L -= 4
        ix <<= 4
    return None


def native_level_ix(level_off, level_n, pos):
    L = FIRST_LEVEL
    for l in range(FIRST_LEVEL + 1, len(level_off)):
        if level_n[l] and pos >= level_off[l]:
            L = l
    return (L, pos - level_off[L])


def walk_heap(q_table, heap_ladder, H, m, zkey, slow):
    """The lookup of the hand-written kernel: one Q entry per index m = 1 (mod 4) -- pre-test, then the first round from its own
    four keys --, later rounds from the heap ladder at sixteen times the position.  slow(m, zkey) answers where the entry has
    level 0.  -> (level, index) or None."""
    if (m & 3) != 1:
        return None
    e = q_table[(m - 1) >> 2]
    if not zkey < int(e["key"]):
        return None
    lvl, pos = int(e["lvl"]), int(e["pos"])
    if lvl == 0:
        return slow(m, zkey)
    four = e["k"]
    while True:
        nf = _first_below(zkey, four)
        pos <<= nf
        if nf < 4:
            level = H - (pos.bit_length() - 1)
            return (level, pos - (1 << (H - level)))
        if lvl < 6:                      # four more levels down would be below level 2
            return None
        lvl -= 4
        four = heap_ladder[pos]


# ---------------------------------------------------------------------------------------------- the shared case set
M_SET = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 4099)
_cases = {}


def zkey_of(z):
    return key_of(z[0], z[1])


class Case:
    """One orbit of M + 1 entries on a built-in view with its host table, the model's view of both and the question set; built
    once per (view, M, type, edit) and shared by the tests, which leave it unchanged."""

    def __init__(self, view_n, M, is64, edit=None, bla_size_exp=None, table_edit=None):
        self.view_n, self.M, self.is64 = view_n, M, is64
        self.view = shallow_view() if view_n == "shallow" else inputs.View.builtin(view_n, 70, 37, antialiasing=1)
        self.orbit = inputs.Orbit(self.view, max_iter=M, periodicity=False, is64=is64)
        assert self.orbit.count == M + 1
        if edit is not None:
            edit(self.orbit)
        self.bla_size = None
        if bla_size_exp is not None:
            self.bla_size = self.orbit.max_radius()
            self.bla_size["e"] += bla_size_exp
        self.bla = inputs.BLATable(self.orbit, bla_size=self.bla_size)   # (built after the edit)
        if table_edit is not None:
            table_edit(self.bla)                                         # (a table no builder makes: for fs_upload_bla only)
        self.tab = Table(self.bla)
        self._qs = self._answers = self._derived = None

    @property
    def questions(self):
        if self._qs is None:
            self._qs = question_set(self.tab, self.orbit.count)
        return self._qs

    @property
    def answers(self):
        if self._answers is None:
            self._answers = answers(self.tab, self.questions)
            self._answers.setflags(write=False)
        return self._answers

    @property
    def derived(self):
        if self._derived is None:
            self._derived = Derived(self.tab, self.orbit.entries())
        return self._derived


def shallow_view():
    """A 70 x 37 view 1e-4 wide off the real axis: short orbits of its centre give frames of hundreds of different counts (the
    frames of the deep built-in views are uniform under an orbit this short)."""
    from decimal import Decimal as D
    cx, cy, w = D("-1.25066"), D("0.02012"), D("1e-4")
    h = w * 37 / 70
    return inputs.View(str(cx - w / 2), str(cy - h / 2), str(cx + w / 2), str(cy + h / 2), 70, 37, num_iterations=20000)


def case(view_n, M, is64=False, edit_name=None, bla_size_exp=None):
    key = (view_n, M, is64, edit_name, bla_size_exp)
    if key not in _cases:
        if edit_name in TABLE_EDITS:
            _cases[key] = Case(view_n, M, is64, None, bla_size_exp, TABLE_EDITS[edit_name])
        else:
            _cases[key] = Case(view_n, M, is64, EDITS[edit_name] if edit_name else None, bla_size_exp)
    return _cases[key]


def _host_level(bla, l):
    """Level l of a host table in place (inputs.BLATable.level hands out a copy)."""
    import ctypes as C
    n = bla.sizes()[l]
    dt = BLA_HDR64_DTYPE if bla.is64 else inputs.BLA_HDR32_DTYPE
    ptrs = (C.c_void_p * bla.num_levels).from_address(bla.level_ptrs)
    buf = (C.c_uint8 * (n * dt.itemsize)).from_address(ptrs[l])
    return np.frombuffer(buf, dtype=dt)


def _table_edit_wide_first_elements(bla):
    """The r2 of the first element of every level above 2 raised by 2^8 and 2^4 alternately.  The builder never makes such a
    table (a merge's r2 is at most its left child's, so the first elements' r2 fall from level to level and the gate of the first
    index -- z2 < r2 of (2, 0) -- is implied by the walk's own probes); in this one the gate decides, and the ladder's keys are
    not monotone."""
    for l in range(FIRST_LEVEL + 1, bla.num_levels):
        _host_level(bla, l)["r2_e"][0] += 8 if (l & 1) else 4


def _edit_arrivals_outside_window(orbit):
    """Orbit entries moved outside 2^-40 .. 2^1 (Orbit.scale_entries / scale_parts): arrival entries above and below the window
    of the quiet forms, and one whose parts lie 200 binades apart."""
    n = orbit.count
    hi = [i for i in (5, 9, 33, n - 2) if 0 < i < n]
    lo = [i for i in (6, 13, 17, 65) if 0 < i < n and i not in hi]
    orbit.scale_entries(hi, [6] * len(hi))
    orbit.scale_entries(lo, [-60] * len(lo))
    far = [i for i in (21,) if i < n]
    orbit.scale_parts(far, [0] * len(far), [-200] * len(far))


EDITS = {"window": _edit_arrivals_outside_window}
TABLE_EDITS = {"wide_first": _table_edit_wide_first_elements}
