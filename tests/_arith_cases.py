"""The committed case set of the arithmetic-edge tests: one op table (the ids of tests/arith/arith_ops.hpp, with the model function of
tests/_ieee_model.py for each entry) and, per family, named generators of edge classes.  Deterministic (random.Random with fixed
seeds); shared by the CPU and the GPU test.

A case is (op name, class name, operands).  Every case keeps every intermediate finite in the model: a draw that does not is drawn
again, and FAMILIES[name].redraws counts how often (the CPU test holds it at 1 % of the family's draws at most).
"""
import math
import random
import struct

import _ieee_model as M
from _ieee_model import F32, F64, R32, R64, RDF, KMIN

IN_WORDS, OUT_WORDS = 16, 8
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1

# ------------------------------------------------------------------------------------------------ words
# type codes: i int32, b bool, f float, d double, D df32; h? hreal, c? hcplx, q? q4, p? pair / dw; A the result of hr_add2


def pack(t, v, out):
    if t == "i" or t == "b":
        out.append(v & 0xFFFFFFFF)
    elif t == "f":
        out.append(F32.bits(v))
    elif t == "d":
        u = F64.bits(v)
        out.extend((u & 0xFFFFFFFF, u >> 32))
    elif t == "D":
        pack("f", v[0], out), pack("f", v[1], out)
    elif t[0] == "h":
        pack(t[1], v[0], out), pack("i", v[1], out)
    elif t[0] == "c":
        pack(t[1], v[0], out), pack(t[1], v[1], out), pack("i", v[2], out)
    elif t[0] in "qp":
        for x in v:
            pack(t[1], x, out)
    elif t == "H":                                   # two hreal<df32>
        pack("hD", v[0], out), pack("hD", v[1], out)
    elif t == "A":
        pack("hD", v[0], out), pack("hD", v[1], out), pack("b", v[2], out)
    else:
        raise ValueError(t)
    return out


def nwords(t):
    if t in "ibf":
        return 1
    if t in "dD":
        return 2
    if t[0] == "h":
        return nwords(t[1]) + 1
    if t[0] == "c":
        return 2 * nwords(t[1]) + 1
    if t[0] == "q":
        return 4 * nwords(t[1])
    if t[0] == "p":
        return 2 * nwords(t[1])
    return {"H": 6, "A": 7}[t]


# ------------------------------------------------------------------------------------------------ the op table
class Op:
    def __init__(self, id_, name, ins, out, fn, host=True):
        self.id, self.name, self.ins, self.out, self.fn, self.host = id_, name, ins, out, fn, host
        self.words_in = sum(nwords(t) for t in ins)
        self.words_out = nwords(out)


OPS = {}


def _op(id_, name, ins, out, fn, host=True):
    assert name not in OPS and all(o.id != id_ for o in OPS.values())
    OPS[name] = Op(id_, name, tuple(ins), out, fn, host)


def _hdr(T, c, S, B, real):
    h, cx = "h" + c, "c" + c
    _op(B + 0, "multiplier_" + S, ["i"], c, T.multiplier)
    _op(B + 1, "multiplier_neg_" + S, ["i"], c, T.multiplier_neg)
    _op(B + 2, "hr_reduce_" + S, [h], h, lambda a: M.hr_reduce(T, a))
    _op(B + 3, "hr_from_mant_" + S, [c], h, lambda a: M.hr_from_mant(T, a))
    _op(B + 5, "hr_mul_" + S, [h, h], h, lambda a, b: M.hr_mul(T, a, b))
    _op(B + 6, "hr_mul2_" + S, [h], h, lambda a: M.hr_mul2(T, a))
    _op(B + 8, "hr_square_" + S, [h], h, lambda a: M.hr_square(T, a))
    _op(B + 9, "hr_add_" + S, [h, h], h, lambda a, b: M.hr_add(T, a, b))
    _op(B + 10, "hr_sub_" + S, [h, h], h, lambda a, b: M.hr_sub(T, a, b))
    _op(B + 12, "hr_abs_" + S, [h], h, lambda a: M.hr_abs(T, a))
    _op(B + 13, "hr_cmp_pos_" + S, [h, h], "i", lambda a, b: M.hr_cmp_pos(T, a, b))
    _op(B + 14, "hr_cmp_" + S, [h, h], "i", lambda a, b: M.hr_cmp(T, a, b))
    _op(B + 15, "hr_max_pos_" + S, [h, h], h, lambda a, b: M.hr_max_pos(T, a, b))
    _op(B + 16, "hr_min_pos_" + S, [h, h], h, lambda a, b: M.hr_min_pos(T, a, b))
    _op(B + 17, "hr_to_native_" + S, [h], c, lambda a: M.hr_to_native(T, a))
    _op(B + 18, "hc_from_hr_" + S, [h, h], cx, lambda a, b: M.hc_from_hr(T, a, b))
    _op(B + 19, "hc_from_native_" + S, [c, c], cx, lambda a, b: M.hc_from_native(T, a, b))
    _op(B + 20, "hc_add_" + S, [cx, cx], cx, lambda a, b: M.hc_add(T, a, b))
    _op(B + 21, "hc_add_real_" + S, [cx, h], cx, lambda a, b: M.hc_add_real(T, a, b))
    _op(B + 22, "hc_mul_" + S, [cx, cx], cx, lambda a, b: M.hc_mul(T, a, b))
    _op(B + 23, "hc_mul_real_" + S, [cx, h], cx, lambda a, b: M.hc_mul_real(T, a, b))
    _op(B + 24, "hc_mul2_" + S, [cx], cx, lambda a: M.hc_mul2(T, a))
    _op(B + 25, "hc_reduce_" + S, [cx], cx, lambda a: M.hc_reduce(T, a))
    _op(B + 26, "hc_norm2_" + S, [cx], h, lambda a: M.hc_norm2(T, a))
    _op(B + 27, "hc_cheb_" + S, [cx], h, lambda a: M.hc_cheb(T, a))
    if real:
        _op(B + 4, "hr_from_number_" + S, [c], h, lambda a: M.hr_from_number(T, a))
        _op(B + 7, "hr_div_" + S, [h, h], h, lambda a, b: M.hr_div(T, a, b))
        _op(B + 11, "hr_recip_" + S, [h], h, lambda a: M.hr_recip(T, a))
        _op(B + 28, "hc_norm_" + S, [cx], h, lambda a: M.hc_norm(T, a))
        _op(B + 29, "hc_div_" + S, [cx, cx], cx, lambda a, b: M.hc_div(T, a, b))
        _op(B + 30, "hc_recip_" + S, [cx], cx, lambda a: M.hc_recip(T, a))


_hdr(R32, "f", "f32", 0, True)
_hdr(R64, "d", "f64", 40, True)
_hdr(RDF, "D", "df32", 80, False)

_op(120, "df32_add", ["D", "D"], "D", RDF.add)
_op(121, "df32_sub", ["D", "D"], "D", RDF.sub)
_op(122, "df32_neg", ["D"], "D", RDF.neg)
_op(123, "df32_mul", ["D", "D"], "D", RDF.mul)
_op(124, "df32_lt", ["D", "D"], "b", lambda a, b: int(RDF.lt(a, b)))
_op(125, "df32_eq", ["D", "D"], "b", lambda a, b: int(RDF.eq(a, b)))
_op(126, "df32_gt", ["D", "D"], "b", lambda a, b: int(RDF.gt(a, b)))
_op(127, "df32_ge", ["D", "D"], "b", lambda a, b: int(RDF.ge(a, b)))
_op(128, "df32_le", ["D", "D"], "b", lambda a, b: int(RDF.le(a, b)))
_op(129, "df32_fabs", ["D"], "D", RDF.fabs)
_op(130, "hr2_from_float", ["f"], "hD", M.hr2_from_float)


def _qd(f, c, S, B):
    q, p = "q" + c, "p" + c
    _op(B + 0, "q_quick_two_sum_" + S, [c, c], p, lambda a, b: M.q_quick_two_sum(f, a, b))
    _op(B + 1, "q_two_sum_" + S, [c, c], p, lambda a, b: M.q_two_sum(f, a, b))
    _op(B + 2, "q_split_" + S, [c], p, lambda a: M.q_split(f, a))
    _op(B + 3, "q_two_prod_" + S, [c, c], p, lambda a, b: M.q_two_prod(f, a, b))
    _op(B + 4, "q_two_sqr_" + S, [c], p, lambda a: M.q_two_sqr(f, a))
    _op(B + 5, "q_renorm_" + S, [q, c], q, lambda a, b: M.q_renorm(f, a[0], a[1], a[2], a[3], b))
    _op(B + 6, "q_add_" + S, [q, q], q, lambda a, b: M.q_add(f, a, b))
    _op(B + 7, "q_sub_" + S, [q, q], q, lambda a, b: M.q_sub(f, a, b))
    _op(B + 8, "q_mul_scalar_" + S, [q, c], q, lambda a, b: M.q_mul_scalar(f, a, b))
    _op(B + 9, "q_mul_" + S, [q, q], q, lambda a, b: M.q_mul(f, a, b))
    _op(B + 10, "q_sqr_" + S, [q], q, lambda a: M.q_sqr(f, a))
    _op(B + 11, "q_mul_pwr2_" + S, [q, c], q, lambda a, b: M.q_mul_pwr2(f, a, b))
    _op(B + 12, "q_le_" + S, [q, q], "b", lambda a, b: M.q_le(f, a, b))
    _op(B + 13, "q_le_scalar_" + S, [q, c], "b", lambda a, b: M.q_le_scalar(f, a, b))


_qd(F32, "f", "f32", 140)
_qd(F64, "d", "f64", 170)

_op(200, "bla_sqrt_f32", ["hf"], "hf", lambda a: M.bla_sqrt(R32, a))
_op(201, "bla_hypot_f32", ["hf", "hf"], "hf", lambda a, b: M.bla_hypot(R32, a, b))
_op(202, "bla_sqrt_f64", ["hd"], "hd", lambda a: M.bla_sqrt(R64, a))
_op(203, "bla_hypot_f64", ["hd", "hd"], "hd", lambda a, b: M.bla_hypot(R64, a, b))


def _dw(f, c, S, B):
    p = "p" + c
    _op(B + 0, "dw_two_sum_" + S, [c, c], p, lambda a, b: M.dw_two_sum(f, a, b), host=False)
    _op(B + 1, "dw_add_" + S, [p, p], p, lambda a, b: M.dw_add(f, a, b), host=False)
    _op(B + 2, "dw_sub_" + S, [p, p], p, lambda a, b: M.dw_sub(f, a, b), host=False)
    _op(B + 3, "dw_mul_" + S, [p, p], p, lambda a, b: M.dw_mul(f, a, b), host=False)
    _op(B + 4, "dw_sqr_" + S, [p], p, lambda a: M.dw_sqr(f, a), host=False)


_dw(F32, "f", "f32", 210)
_op(215, "dw_mul2x_f32", ["pf", "pf"], "pf", lambda a, b: M.dw_mul2x(F32, a, b), host=False)
_dw(F64, "d", "f64", 220)
_op(230, "fma_down_f32", ["f", "f", "f"], "f", lambda a, b, c: M.fma_down(F32, a, b, c), host=False)


def _add2(minus):
    """hr_add2<kSubLo>: x is a.x -/+ b.x, y is a.y + b.y; `rare` where a result is zero (the straight line leaves those, and the
    non-finite ones, to its caller's literal path, and what it returns for them is not pinned)"""
    def fn(a, b):
        x = (M.hr_sub if minus else M.hr_add)(RDF, a[0], b[0])
        y = M.hr_add(RDF, a[1], b[1])
        return (x, y, int(x[0][0] == 0 or y[0][0] == 0))
    return fn


_op(240, "hr_add2_add", ["H", "H"], "A", _add2(False), host=False)
_op(241, "hr_add2_sub", ["H", "H"], "A", _add2(True), host=False)


# ------------------------------------------------------------------------------------------------ operand draws
def r32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def rfloat(rng, fmt, elo, ehi, sign=None):
    """a random normal value of fmt with exponent in [elo, ehi]"""
    frac = rng.getrandbits(fmt.p - 1)
    v = math.ldexp((1 << (fmt.p - 1)) | frac, rng.randint(elo, ehi) - (fmt.p - 1))
    if sign is None:
        sign = rng.random() < 0.5
    return -v if sign else v


def rsub(rng, fmt):
    """a subnormal of fmt (now and then the smallest or the largest)"""
    k = rng.random()
    n = 1 if k < 0.15 else ((1 << (fmt.p - 1)) - 1 if k < 0.3 else rng.randint(1, (1 << (fmt.p - 1)) - 1))
    v = n * fmt.tiny
    return -v if rng.random() < 0.5 else v


def nextup(fmt, x, n=1):
    """n steps away from zero in fmt (x normal)"""
    return fmt.from_bits(fmt.bits(x) + n)


def rdf(rng, elo, ehi, kind=None):
    """a double-float: the kinds are the classes of the issue (normalised pair, zero tail, tail of opposite sign, tail with a gap)"""
    h = rfloat(rng, F32, elo, ehi)
    kind = kind or rng.choice(("norm", "norm", "zero_tail", "opposite", "gap", "half_ulp"))
    e = math.frexp(h)[1] - 1
    if kind == "zero_tail":
        return (h, 0.0)
    if kind == "half_ulp":
        t = math.ldexp(1.0, e - 24)                     # exactly half an ulp of the head
        return (h, -t if rng.random() < 0.5 else t)
    t = rfloat(rng, F32, e - 25 - (rng.randint(3, 20) if kind == "gap" else rng.randint(0, 2)), e - 25)
    if kind == "opposite":
        t = math.copysign(t, -h)
    if abs(t) < F32.minnorm:
        t = 0.0
    return (h, t)


def rdw(rng, fmt, elo, ehi, kind=None):
    """as rdf for dw<T>"""
    if fmt is F32:
        return rdf(rng, elo, ehi, kind)
    h = rfloat(rng, fmt, elo, ehi)
    kind = kind or rng.choice(("norm", "norm", "zero_tail", "opposite", "gap", "half_ulp"))
    e = math.frexp(h)[1] - 1
    if kind == "zero_tail":
        return (h, 0.0)
    if kind == "half_ulp":
        t = math.ldexp(1.0, e - fmt.p)
        return (h, -t if rng.random() < 0.5 else t)
    t = rfloat(rng, fmt, e - fmt.p - 1 - (rng.randint(3, 20) if kind == "gap" else rng.randint(0, 2)), e - fmt.p - 1)
    if kind == "opposite":
        t = math.copysign(t, -h)
    return (h, t)


class Draw:
    """mantissas of the numeric type T (R32 / R64 / RDF)"""

    def __init__(self, T, rng):
        self.T, self.rng, self.f = T, rng, T.fmt
        self.df = T is RDF

    def norm(self):                                      # in [1, 2), either sign
        return rdf(self.rng, 0, 0) if self.df else rfloat(self.rng, self.f, 0, 0)

    def unnorm(self, span=40):
        return rdf(self.rng, -span, span) if self.df else rfloat(self.rng, self.f, -span, span)

    def sub(self):
        v = rsub(self.rng, self.f)
        return (v, 0.0) if self.df else v

    def zero(self):
        z = -0.0 if self.rng.random() < 0.5 else 0.0
        return (z, z if self.rng.random() < 0.5 else 0.0) if self.df else z

    def any(self):
        k = self.rng.random()
        return self.norm() if k < 0.4 else (self.unnorm() if k < 0.8 else (self.sub() if k < 0.95 else self.zero()))

    def scale(self, m, s):
        """m * 2^s, exact where nothing underflows"""
        if self.df:
            return (r32(math.ldexp(m[0], s)), r32(math.ldexp(m[1], s)))
        return math.ldexp(m, s) if self.f is F64 else r32(math.ldexp(m, s))

    def neg(self, m):
        return (-m[0], -m[1]) if self.df else -m

    def near(self, m):
        """m moved by one unit of its last place"""
        if self.df:
            return (m[0], nextup(F32, m[1]) if m[1] != 0 else math.copysign(math.ldexp(abs(m[0]), -47), m[0]))
        return nextup(self.f, m)

    def exp(self):
        k = self.rng.random()
        if k < 0.5:
            return self.rng.randint(-2000, 2000)
        if k < 0.8:
            return self.rng.randint(-(1 << 26), 1 << 26)
        return KMIN + self.rng.randint(0, 400)


GAPS = (-130, -121, -120, -119, -1, 0, 1, 119, 120, 121, 130)


def gaps_for(T):
    return GAPS + ((-1023, -1022) if T is R64 else (-127, -126)) + ((127, 126) if T is not R64 else (1023, 1022))


# ------------------------------------------------------------------------------------------------ class generators
# each yields (op name, operands); the family runner names the class after the generator

def g_gaps(T, S, rng, n):
    """exponent gaps of the four adds / subs, crossed with equal / opposite / nearly opposite / unrelated mantissas"""
    D = Draw(T, rng)
    for _ in range(n):
        for gap in gaps_for(T):
            for rel in ("equal", "opposite", "nearly_opposite", "unrelated", "same_bits"):
                for op in ("hr_add", "hr_sub", "hc_add", "hc_add_real"):
                    base = D.exp() if rng.random() < 0.7 else 0
                    if base + gap < INT_MIN + 2000 or base < KMIN - 100000:
                        base = 0
                    am = D.norm() if rng.random() < 0.7 else D.unnorm(3)
                    s = gap if abs(gap) < 120 else 0
                    if rel == "equal":
                        bm = D.scale(am, s)
                    elif rel == "opposite":
                        bm = D.neg(D.scale(am, s))
                    elif rel == "nearly_opposite":
                        bm = D.neg(D.near(D.scale(am, s)))
                    elif rel == "same_bits":
                        bm = am
                    else:
                        bm = D.unnorm(3)
                    ae, be = base + gap, base
                    if op in ("hr_add", "hr_sub"):
                        yield op + "_" + S, ((am, ae), (bm, be))
                    elif op == "hc_add":
                        yield op + "_" + S, ((am, D.any() if rng.random() < 0.5 else D.neg(am), ae),
                                             (bm, D.unnorm(3), be))
                    else:
                        yield op + "_" + S, ((am, D.any(), ae), (bm, be))


def g_zero_mantissa(T, S, rng, n):
    """a zero mantissa on either side at exponent 0, at an arbitrary exponent and at kMinBigExp"""
    D = Draw(T, rng)
    for _ in range(n):
        for gap in GAPS:
            for ze in (0, rng.randint(-5000, 5000), KMIN):
                for side in (0, 1, 2):
                    for op in ("hr_add", "hr_sub", "hc_add", "hc_add_real"):
                        za = D.zero() if side in (0, 2) else D.any()
                        zb = D.zero() if side in (1, 2) else D.any()
                        ae, be = (ze, ze - gap) if side in (0, 2) else (ze + gap, ze)
                        if op in ("hr_add", "hr_sub"):
                            yield op + "_" + S, ((za, ae), (zb, be))
                        elif op == "hc_add":
                            yield op + "_" + S, ((za, D.zero() if rng.random() < 0.5 else D.any(), ae), (zb, D.zero(), be))
                        else:
                            yield op + "_" + S, ((za, D.zero(), ae), (zb, be))


def g_exp_cross(T, S, rng, n):
    """exponent sums and differences that cross kMinBigExp in the products and quotients"""
    D = Draw(T, rng)
    real = T is not RDF
    for _ in range(n):
        for k in (-3, -2, -1, 0, 1, 2, rng.randint(-1000, 1000)):
            split = rng.randint(0, 1 << 27)
            ae, be = KMIN + split + k, -split             # ae + be = KMIN + k
            yield "hr_mul_" + S, ((D.norm(), ae), (D.norm(), be))
            yield "hc_mul_" + S, ((D.norm(), D.norm(), ae), (D.norm(), D.norm(), be))
            yield "hc_mul_real_" + S, ((D.norm(), D.norm(), ae), (D.norm(), be))
            yield "hr_mul2_" + S, ((D.norm(), KMIN - 1 + k),)
            yield "hc_mul2_" + S, ((D.norm(), D.norm(), KMIN - 1 + k),)
            if real:
                yield "hr_div_" + S, ((D.norm(), ae), (D.norm(), -be))
                yield "hc_div_" + S, ((D.norm(), D.norm(), ae), (D.norm(), D.norm(), -be))


def g_square_wrap(T, S, rng, n):
    """hr_square and hc_norm2 do not clamp: exponents whose doubling wraps in 32 bits"""
    D = Draw(T, rng)
    for _ in range(n):
        for e in (1 << 30, (1 << 30) - 1, (1 << 30) + 5, -(1 << 30), -(1 << 30) - 1, INT_MAX, INT_MIN, 3 << 29, KMIN, KMIN - 7,
                  rng.randint(INT_MIN, INT_MAX), rng.randint(-1000, 1000)):
            yield "hr_square_" + S, ((D.norm(), e),)
            yield "hc_norm2_" + S, ((D.norm(), D.norm(), e),)


def g_mantissas(T, S, rng, n):
    """every function on normalised, unnormalised (+-40 binades), subnormal and zero mantissas"""
    D = Draw(T, rng)
    real = T is not RDF
    for _ in range(n):
        h = lambda: (D.any(), D.exp())
        hsmall = lambda: (D.any(), rng.randint(-150, 150))
        c = lambda: (D.any(), D.any(), D.exp())
        for op, args in (("hr_reduce", (h(),)), ("hr_from_mant", (D.any(),)), ("hr_mul", (h(), h())), ("hr_mul2", (h(),)),
                         ("hr_square", ((D.any(), rng.randint(-1 << 20, 1 << 20)),)), ("hr_add", (hsmall(), hsmall())),
                         ("hr_sub", (hsmall(), hsmall())), ("hr_abs", (h(),)), ("hr_to_native", ((D.any(), rng.randint(-150, 80)),)),
                         ("hc_from_hr", (hsmall(), hsmall())), ("hc_from_native", (D.any(), D.any())),
                         ("hc_add", ((D.any(), D.any(), rng.randint(-150, 150)), (D.any(), D.any(), rng.randint(-150, 150)))),
                         ("hc_add_real", ((D.any(), D.any(), rng.randint(-150, 150)), hsmall())),
                         ("hc_mul", (c(), c())), ("hc_mul_real", (c(), h())), ("hc_mul2", (c(),)), ("hc_reduce", (c(),)),
                         ("hc_norm2", ((D.any(), D.any(), rng.randint(-1 << 20, 1 << 20)),)), ("hc_cheb", (c(),))):
            yield op + "_" + S, args
        if real:
            v = D.any()
            yield "hr_from_number_" + S, (v,)
            yield "hc_norm_" + S, (c(),)


def g_compare(T, S, rng, n):
    """the comparisons: ties in the exponent, in the mantissa, zeros of either sign"""
    D = Draw(T, rng)
    for _ in range(n):
        for rel in ("same", "exp", "mant", "zero_a", "zero_b", "zero_both", "neg_both", "near"):
            e = D.exp()
            a = (D.unnorm(3), e)
            if rel == "same":
                b = a
            elif rel == "exp":
                b = (a[0], e + rng.choice((-1, 1)))
            elif rel == "mant":
                b = (D.unnorm(3), e)
            elif rel == "near":
                b = (D.near(a[0]), e)
            elif rel == "zero_a":
                a, b = (D.zero(), e), (D.unnorm(3), D.exp())
            elif rel == "zero_b":
                b = (D.zero(), D.exp())
            elif rel == "zero_both":
                a, b = (D.zero(), e), (D.zero(), D.exp())
            else:
                a = (D.neg(D.T.fabs(a[0])), e)
                b = (D.neg(D.T.fabs(D.unnorm(3))), e + rng.choice((-1, 0, 0, 1)))
            yield "hr_cmp_" + S, (a, b)
            pa, pb = (D.T.fabs(a[0]), a[1]), (D.T.fabs(b[0]), b[1])
            for op in ("hr_cmp_pos", "hr_max_pos", "hr_min_pos"):
                yield op + "_" + S, (pa, pb)


def g_multiplier(T, S, rng, n):
    """multiplier / multiplier_neg at their cut-offs, and hr_to_native's type_max saturation"""
    D = Draw(T, rng)
    f = T.fmt
    edge = (-f.bias - 1, -f.bias, -f.bias + 1, -f.bias + 2, -1, 0, 1, f.emax - 1, f.emax, f.emax + 1, f.emax + 2,
            -1023, -1022, -127, -126, 127, 128, 1023, 1024, KMIN, INT_MIN, INT_MAX, 1 << 24, -(1 << 24))
    for s in edge + tuple(rng.randint(-1100, 1100) for _ in range(n)):
        yield "multiplier_" + S, (s,)
        if s <= f.emax:
            yield "multiplier_neg_" + S, (s,)
    for _ in range(n):
        # type_max times a mantissa at most 1 stays finite; the largest finite mantissa with exponent 0 is itself
        m = D.scale(D.norm(), -rng.randint(1, 30))
        yield "hr_to_native_" + S, ((m, rng.choice((f.emax + 1, f.emax + 2, 5000, INT_MAX))),)
        yield "hr_to_native_" + S, ((m, rng.choice((f.emax, f.emax - 1, f.emax - 3)) - 30),)
        yield "hr_to_native_" + S, ((D.norm(), rng.choice((-f.bias + 1, -f.bias, -f.bias - 1, -f.bias + 2, -f.bias - 22, KMIN))),)
        big = (f.max, 0.0) if T is RDF else f.max
        yield "hr_to_native_" + S, ((D.neg(big) if rng.random() < 0.5 else big, rng.choice((0, 0, -1, -5))),)
        yield "hr_reduce_" + S, ((big, D.exp()),)


def g_subnormal_products(T, S, rng, n):
    """products and scaled terms that land in the subnormal range and exactly on its edges"""
    D = Draw(T, rng)
    f = T.fmt
    wrapm = (lambda v: (v, 0.0)) if T is RDF else (lambda v: v)
    for _ in range(n):
        for target in (f.emin - f.p + 1, f.emin - f.p, f.emin - f.p + 2, f.emin, f.emin - 1, f.emin + 1,
                       rng.randint(f.emin - f.p - 1, f.emin + 1)):
            ea = target // 2 + rng.randint(-10, 10)
            a = rfloat(rng, f, ea, ea)
            b = rfloat(rng, f, target - ea, target - ea)
            pw = rng.random() < 0.3
            if pw:                                           # powers of two: the product sits exactly on the edge
                a, b = math.ldexp(1.0, ea), math.ldexp(1.0, target - ea)
            yield "hr_mul_" + S, ((wrapm(a), 0), (wrapm(b), D.exp()))
            yield "hr_square_" + S, ((wrapm(rfloat(rng, f, target // 2, target // 2)), 7),)
            yield "hc_mul_" + S, ((wrapm(a), wrapm(-a), 3), (wrapm(b), wrapm(b), -3))
            yield "hc_mul_real_" + S, ((wrapm(a), D.norm(), 3), (wrapm(b), -3))
            yield "hc_norm2_" + S, ((wrapm(rfloat(rng, f, target // 2, target // 2)), wrapm(rfloat(rng, f, target // 2 - 1, target // 2)), 0),)
            # a scaled term of an add that lands there: b.m * 2^-gap
            eb = rng.randint(f.emin, f.emin + 20)
            gap = eb - target                                 # 0 < gap < 120 for both formats
            yield "hr_add_" + S, ((D.sub() if rng.random() < 0.5 else wrapm(rfloat(rng, f, f.emin, f.emin + 3)), gap),
                                  (wrapm(rfloat(rng, f, eb, eb)), 0))
            yield "hr_sub_" + S, ((wrapm(rfloat(rng, f, eb, eb)), -gap), (D.sub(), 0))
            yield "hc_add_" + S, ((wrapm(rfloat(rng, f, eb, eb)), D.sub(), -gap), (D.sub(), D.sub(), 0))
            yield "hr_to_native_" + S, ((wrapm(rfloat(rng, f, 0, 0)), target),)
            yield "hc_from_hr_" + S, ((wrapm(rfloat(rng, f, 0, 0)), target + 50), (D.norm(), 50))


def g_reduce(T, S, rng, n):
    """hr_reduce / hc_reduce / hc_from_hr: one component zero, both subnormal, components 200 binades apart, zeros that keep or
    reset the exponent; for df32 the tail's saturating exponent shift"""
    D = Draw(T, rng)
    f = T.fmt
    wrapm = (lambda v: (v, 0.0)) if T is RDF else (lambda v: v)
    real = T is not RDF
    for _ in range(n):
        e = D.exp()
        far = 200 if T is not R64 else rng.choice((200, 1500))
        lo = rng.randint(-far // 2 - 20, -far // 2)
        pairs = ((D.zero(), D.any()), (D.any(), D.zero()), (D.zero(), D.zero()), (D.sub(), D.sub()), (D.sub(), D.zero()),
                 (wrapm(rfloat(rng, f, lo, lo)), wrapm(rfloat(rng, f, lo + far, lo + far))),
                 (wrapm(rfloat(rng, f, lo + far, lo + far)), wrapm(rfloat(rng, f, lo, lo))),
                 (wrapm(f.tiny), wrapm(-f.tiny)), (D.sub(), D.unnorm()), (D.unnorm(), D.unnorm()))
        for re, im in pairs:
            yield "hc_reduce_" + S, ((re, im, e),)
            yield "hc_from_native_" + S, (re, im)
            yield "hc_from_hr_" + S, ((re, rng.randint(-300, 300)), (im, rng.randint(-300, 300)))
            yield "hc_from_hr_" + S, ((re, e), (im, e + rng.choice((0, -1, 1, -f.bias, -f.bias + 1, f.bias, f.bias - 1, 5000, -5000))))
            yield "hr_reduce_" + S, ((re, e),)
            yield "hr_from_mant_" + S, (im,)
            if real:
                yield "hr_from_number_" + S, (re,)
        if T is RDF:
            # zero tail under a head below 1; a tail exponent field smaller than the shift; a negative head
            for h, t in ((rfloat(rng, F32, -60, -1), 0.0), (rfloat(rng, F32, -60, -1), -0.0),
                         (rfloat(rng, F32, 40, 100), rfloat(rng, F32, -126, -100)),
                         (rfloat(rng, F32, 40, 100), rsub(rng, F32)),
                         (rfloat(rng, F32, -60, 60, sign=True), rfloat(rng, F32, -100, -90)),
                         (rfloat(rng, F32, 1, 60, sign=True), 0.0), (0.0, rfloat(rng, F32, -120, -60)),
                         (rsub(rng, F32), 0.0), rdf(rng, -60, 60)):
                yield "hr_reduce_df32", (((h, t), e),)
                yield "hr_from_mant_df32", ((h, t),)
                yield "hc_reduce_df32", (((h, t), rdf(rng, -60, 60), e),)
                yield "hc_reduce_df32", ((D.zero(), (h, t), e),)


def near_tie_quotient(rng, fmt):
    """(a, b) with a / b within 2^-(2p-2) (relative) of a rounding tie of fmt: a * 2^(p+1) = Mo * b + r with Mo odd and of p + 1
    bits, r = +-1"""
    p = fmt.p
    while True:
        b = rng.getrandbits(p - 1) | (1 << (p - 1)) | 1
        r = rng.choice((-1, 1))
        Mo = (-r * pow(b, -1, 1 << (p + 1))) % (1 << (p + 1))
        if Mo < (1 << p):
            continue
        a = (Mo * b + r) >> (p + 1)
        assert (a << (p + 1)) == Mo * b + r and a < (1 << p)
        if a >= (1 << (p - 1)):
            return float(a), float(b)


def near_tie_radicand(rng, fmt):
    """x in [1, 4) whose root lies within j^2 2^-(2p+1) <= 2^-(2p-7) (relative) of a rounding tie, for an odd j < 16: the root of
    1 + j 2^-(p-1) is 1 + j 2^-p - j^2 2^-(2p+1) - ..., and 1 + j 2^-p is a tie of p bits; the root of 4 (1 - j 2^-p) is
    2 (1 - j 2^-(p+1) - j^2 2^-(2p+3) - ...), and 1 - j 2^-(p+1) is a tie below 1.  A power of 4 as a factor keeps both."""
    p = fmt.p
    j = rng.randrange(1, 16, 2)
    if rng.random() < 0.5:
        return math.ldexp((1 << (p - 1)) + j, -(p - 1))          # just above 1
    return math.ldexp((1 << p) - j, -p + 2)                      # just below 4


def g_div_sqrt(T, S, rng, n):
    """quotients and radicands within 2^-40 (binary32) / 2^-80 (binary64) of a rounding tie, subnormal quotients, odd and even
    (also negative) exponents of bla_sqrt"""
    D = Draw(T, rng)
    f = T.fmt
    for _ in range(n):
        a, b = near_tie_quotient(rng, f)
        sa, sb = rng.randint(-30, 30), rng.randint(-30, 30)
        a, b = math.ldexp(a, sa - f.p) * rng.choice((-1, 1)), math.ldexp(b, sb - f.p) * rng.choice((-1, 1))
        yield "hr_div_" + S, ((a, D.exp()), (b, rng.randint(-2000, 2000)))
        yield "hr_div_" + S, ((D.unnorm(30), D.exp()), (D.unnorm(30), rng.randint(-2000, 2000)))
        # subnormal quotients, the near tie included
        down = rng.randint(f.emin - f.p - 2, f.emin + 1)
        yield "hr_div_" + S, ((math.ldexp(a, down // 2 - sa), 0), (math.ldexp(b, -(down - down // 2) - sb), 0))
        yield "hr_div_" + S, ((rfloat(rng, f, down // 2, down // 2), 0), (rfloat(rng, f, -(down - down // 2), -(down - down // 2)), 0))
        yield "hr_recip_" + S, ((D.unnorm(40), D.exp()),)
        yield "hr_recip_" + S, ((rfloat(rng, f, f.emax - 3, f.emax - 1), 3),)          # a subnormal reciprocal
        yield "hc_div_" + S, ((D.unnorm(20), D.unnorm(20), D.exp()), (D.unnorm(20), D.unnorm(20), rng.randint(-2000, 2000)))
        yield "hc_div_" + S, ((D.unnorm(20), D.zero(), D.exp()), (D.zero(), D.unnorm(20), 5))
        yield "hc_recip_" + S, ((D.unnorm(20), D.unnorm(20), D.exp()),)
        yield "hc_recip_" + S, ((D.zero(), D.unnorm(20), D.exp()),)
        yield "hc_norm_" + S, ((D.unnorm(40), D.unnorm(40), D.exp()),)
        yield "hc_norm_" + S, ((D.sub(), D.sub(), D.exp()),)


def g_bla(T, S, rng, n):
    """bla_sqrt at odd and even exponents of either sign, radicands near a rounding tie, subnormal radicands; bla_hypot"""
    D = Draw(T, rng)
    f = T.fmt
    for _ in range(n):
        for e in (0, 1, -1, 2, -2, 3, -3, KMIN, KMIN + 1, rng.randint(-5000, 5000), rng.randint(-5000, 5000) | 1,
                  -(rng.randint(0, 5000) | 1)):
            x = near_tie_radicand(rng, f)
            v = math.ldexp(x, 2 * rng.randint(-20, 20))
            yield "bla_sqrt_" + S, ((v / 2 if e & 1 else v, e),)         # the radicand is 2 m at an odd exponent
            yield "bla_sqrt_" + S, ((abs(D.unnorm(40)), e),)
        yield "bla_sqrt_" + S, ((abs(D.sub()), rng.randint(-9, 9)),)
        yield "bla_sqrt_" + S, ((0.0, rng.randint(-9, 9)),)
        yield "bla_hypot_" + S, ((D.unnorm(20), D.exp()), (D.unnorm(20), rng.randint(-2000, 2000)))
        e = rng.randint(-3000, 3000)
        yield "bla_hypot_" + S, ((D.unnorm(20), e), (D.unnorm(20), e + rng.randint(-62, 62)))
        yield "bla_hypot_" + S, ((D.zero(), e), (D.unnorm(20), e + rng.randint(-3, 3)))


def _pairs(rng, fmt, mk):
    """operand pairs of a double-word type over +-60 binades"""
    return mk(rng, fmt, -60, 60), mk(rng, fmt, -60, 60)


def g_dw_pairs(prefix, fmt, S, rng, n, ops):
    """normalised pairs over +-60 binades: zero tails, tails of opposite sign, tails with a gap, half-ulp tails"""
    for _ in range(n):
        a, b = _pairs(rng, fmt, rdw)
        for op in ops:
            yield prefix + op + S, (a, b)


def g_dw_cancel(prefix, fmt, S, rng, n, ops):
    """exact and near cancellation"""
    for _ in range(n):
        a = rdw(rng, fmt, -60, 60)
        kind = rng.choice(("exact", "head", "near", "near_tail"))
        if kind == "exact":
            b = a
        elif kind == "head":
            b = (a[0], a[1] * rng.choice((0.5, 2.0, -1.0)))
        elif kind == "near":
            b = (nextup(fmt, a[0], rng.randint(1, 3)), a[1])
        else:
            b = (a[0], nextup(fmt, a[1]) if a[1] != 0 else math.ldexp(a[0], -2 * fmt.p))
        for op in ops:
            yield prefix + op + S, (a, b)                       # a - b cancels
            yield prefix + op + S, (a, (-b[0], -b[1]))          # a + (-b) cancels


def g_dw_exact_products(prefix, fmt, S, rng, n, ops):
    """a head product that is exact (the error term is +-0) and products whose error term is subnormal"""
    p = fmt.p
    for _ in range(n):
        ha = math.ldexp(rng.getrandbits(p // 2 - 1) | 1, rng.randint(-30, 30)) * rng.choice((-1, 1))
        hb = math.ldexp(rng.getrandbits(p // 2 - 1) | 1, rng.randint(-30, 30)) * rng.choice((-1, 1))
        for a, b in (((ha, 0.0), (hb, 0.0)), ((ha, -0.0), (hb, 0.0)), ((ha, 0.0), (math.ldexp(1.0, rng.randint(-30, 30)), -0.0)),
                     ((ha, math.ldexp(ha, -p - 3)), (hb, 0.0))):
            for op in ops:
                yield prefix + op + S, (a, b)
        # the error of the head product is about 2^-p of it: put the product near 2^(emin + p) and below
        tgt = rng.randint(fmt.emin - 2, fmt.emin + p + 3)
        ea = tgt // 2 + rng.randint(-5, 5)
        a = (rfloat(rng, fmt, ea, ea), 0.0)
        b = (rfloat(rng, fmt, tgt - ea, tgt - ea), 0.0)
        for op in ops:
            yield prefix + op + S, (a, b)


def g_df32_compare(rng, n):
    """the five comparisons and fabs_bits<df32>: ties in the head, in the tail, zeros of either sign"""
    for _ in range(n):
        a = rdf(rng, -60, 60)
        for b in (a, (a[0], -a[1]), (a[0], nextup(F32, a[1]) if a[1] else math.ldexp(1.0, -100)), (nextup(F32, a[0]), a[1]), rdf(rng, -60, 60),
                  (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-a[0], -a[1]), (-a[0], a[1])):
            for op in ("lt", "eq", "gt", "ge", "le"):
                yield "df32_" + op, (a, b)
                yield "df32_" + op, (b, a)
            yield "df32_fabs", (b,)
            yield "df32_neg", (b,)
        yield "df32_fabs", ((0.0, rfloat(rng, F32, -60, 0)),)      # a zero head: the tail decides
        yield "df32_fabs", ((-0.0, rfloat(rng, F32, -60, 0)),)
        v = rng.choice((0.0, -0.0, rsub(rng, F32), rfloat(rng, F32, -126, 127), F32.max, -F32.tiny))
        yield "hr2_from_float", (v,)


def g_fma_down(rng, n):
    """the fused multiply-add toward -infinity: exact results, results just above / below a representable value in both signs,
    ties, exact-zero sums, subnormal results"""
    f = F32
    for _ in range(n):
        a, b = rfloat(rng, f, -20, 20), rfloat(rng, f, -20, 20)
        A, B = rng.getrandbits(11) | 1, rng.getrandbits(11) | 1
        ea, eb = rng.randint(-20, 20), rng.randint(-20, 20)
        xa, xb = math.ldexp(A, ea) * rng.choice((-1, 1)), math.ldexp(B, eb) * rng.choice((-1, 1))
        prod = xa * xb                                            # exact: 22 bits
        big = math.ldexp(1.0, math.frexp(prod)[1] + 30) * rng.choice((-1, 1))
        yield "exact", (xa, xb, math.ldexp(rng.getrandbits(10), ea + eb) * rng.choice((-1, 1)))
        yield "exact_zero_sum", (xa, xb, -prod)                   # -0 toward -infinity, +0 to nearest
        yield "exact_zero_sum", (0.0, xb, -0.0)
        yield "exact_zero_sum", (-0.0, xb, 0.0 if xb > 0 else -0.0)
        yield "exact_zero_sum", (0.0, xb, 0.0)
        yield "exact_zero_sum", (-0.0, abs(xb), -0.0)
        yield "just_off_representable", (xa, xb, big)             # a large addend: the product is a crumb of either sign under it
        yield "just_off_representable", (a, b, big)
        # and the other way round: the exact 22-bit product with a crumb of either sign under it
        yield "just_off_representable", (xa, xb, math.ldexp(1.0, math.frexp(prod)[1] - 40) * rng.choice((-1, 1)))
        # an exact tie of round-to-nearest: c = (24 bits) * u, the product u / 2 or 3 u / 2 exactly (u the unit of c)
        u = math.ldexp(1.0, rng.randint(-20, 20))
        c = (rng.getrandbits(23) | (1 << 23)) * u
        yield "tie", (0.5, u * rng.choice((-1, 1)), c * rng.choice((-1, 1)))
        yield "tie", (1.5, u * rng.choice((-1, 1)), c * rng.choice((-1, 1)))
        yield "random", (a, b, rfloat(rng, f, -45, 45))
        # subnormal results, and crumbs under the smallest subnormal in both signs
        t = rng.randint(-160, -120)
        yield "subnormal", (rfloat(rng, f, -70, -60), rfloat(rng, f, t + 60, t + 65), rsub(rng, f))
        yield "subnormal", (rfloat(rng, f, -80, -76), rfloat(rng, f, -80, -76), rng.choice((0.0, -0.0, f.tiny, -f.tiny)))
        yield "subnormal", (f.tiny * rng.choice((-1, 1)), rng.choice((0.5, 0.25, 0.75, 1.5)), rsub(rng, f))


def rq4(rng, fmt, e0, nz=4, gapped=False):
    """a four-word expansion of fmt with head exponent e0: each word at most half a unit of the one before; the last 4 - nz words
    zero; `gapped` leaves binades between the words"""
    w, e = [], e0
    for i in range(4):
        if i >= nz:
            w.append(0.0)
            continue
        w.append(rfloat(rng, fmt, e, e))
        e -= fmt.p + 1 + (rng.randint(2, 30 if fmt is F64 else 8) if gapped else rng.randint(0, 1))
    return tuple(w)


def g_q4(fmt, S, rng, n, heavy):
    """full four-word expansions, the last one / two / three words zero, gapped words; a - b with one to four leading words equal"""
    span = 200 if fmt is F64 else 25
    for i in range(n):
        nz = (4, 4, 3, 2, 1)[i % 5]
        gapped = (i % 7) == 3
        a = rq4(rng, fmt, rng.randint(-span, span), nz, gapped)
        b = rq4(rng, fmt, rng.randint(-span, span) if i % 3 else math.frexp(a[0])[1] - 1 + rng.randint(-2, 2),
                (4, 3, 4, 1, 2, 4)[i % 6], (i % 11) == 5)
        yield "q_add_" + S, (a, b)
        yield "q_sub_" + S, (a, b)
        yield "q_mul_scalar_" + S, (a, b[0])
        yield "q_mul_pwr2_" + S, (a, math.ldexp(1.0, rng.randint(-30, 30)))
        if i % heavy == 0:
            yield "q_mul_" + S, (a, b)
            yield "q_sqr_" + S, (a,)
        k = 1 + i % 4                                              # leading words equal
        c = a[:k] + rq4(rng, fmt, math.frexp(a[0])[1] - 1 - k * (fmt.p + 1) - 1, 4)[:4 - k]
        yield "q_sub_" + S, (a, c)
        yield "q_sub_" + S, (a, a)
        yield "q_le_" + S, (a, c)
        yield "q_le_" + S, (c, a)
        yield "q_le_" + S, (a, a)
        yield "q_le_" + S, (a, b)
        yield "q_le_" + S, (b, a)
        for y in (0.0, -0.0, a[1], -a[1] if a[1] else math.ldexp(1.0, -100)):
            yield "q_le_scalar_" + S, ((a[0], y, a[2], a[3]), a[0])
        yield "q_le_scalar_" + S, (a, b[0])
        yield "q_le_scalar_" + S, (a, nextup(fmt, a[0]))


def g_q4_pieces(fmt, S, rng, n):
    """the error-free pieces: two-sums with a zero operand, splits and products of full-width operands, renormalisation of
    overlapping, zero-ridden and already-normalised five-term inputs"""
    span = 200 if fmt is F64 else 25
    p = fmt.p
    for i in range(n):
        a, b = rfloat(rng, fmt, -span, span), rfloat(rng, fmt, -span, span)
        if abs(a) < abs(b):
            a, b = b, a
        z = rng.choice((0.0, -0.0))
        for x, y in ((a, b), (a, z), (z, z), (a, -a), (a, math.ldexp(b, -p - 3))):
            yield "q_quick_two_sum_" + S, (x, y)
            yield "q_two_sum_" + S, (x, y)
            yield "q_two_sum_" + S, (y, x)
        yield "q_split_" + S, (a,)
        yield "q_split_" + S, (math.ldexp(rng.getrandbits(p // 2 - 2) | 1, rng.randint(-span, span)),)   # lo is zero
        yield "q_two_prod_" + S, (a, b)
        yield "q_two_sqr_" + S, (a,)
        yield "q_two_prod_" + S, (a, math.ldexp(1.0, rng.randint(-20, 20)))
        # renormalisation
        e0 = rng.randint(-span, span)
        full = rq4(rng, fmt, e0, 4) + (rfloat(rng, fmt, e0 - 4 * p - 6, e0 - 4 * p - 5),)
        step = p - rng.randint(1, 6)                                # neighbouring words overlap by 1 .. 6 bits
        over = tuple(rfloat(rng, fmt, e0 - j * step, e0 - j * step) for j in range(5))
        yield "q_renorm_" + S, (full[:4], full[4])
        yield "q_renorm_" + S, (over[:4], over[4])
        pat = rng.getrandbits(5)
        zr = tuple((full[j] if (pat >> j) & 1 else 0.0) for j in range(5))
        yield "q_renorm_" + S, (zr[:4], zr[4])
        # words that cancel in the first pass, so the second pass meets zeros in the middle
        yield "q_renorm_" + S, ((full[0], full[1], -full[1], full[3]), full[4])
        yield "q_renorm_" + S, ((full[0], -full[0], full[2], 0.0), rng.choice((0.0, full[4])))
        yield "q_renorm_" + S, ((full[0], 0.0, 0.0, full[3]), full[4])
        yield "q_renorm_" + S, ((full[0], 0.0, full[2], 0.0), rng.choice((0.0, full[4])))
        yield "q_renorm_" + S, ((full[0], full[1], 0.0, 0.0), rng.choice((0.0, full[4])))
        yield "q_renorm_" + S, ((full[0], 0.0, 0.0, 0.0), rng.choice((0.0, full[4])))
        yield "q_renorm_" + S, ((0.0, 0.0, 0.0, 0.0), rng.choice((0.0, full[4])))


def g_q4_double_high(rng, n):
    """q4<double> heads above 2^996: the scaled arm of q_split, in q_two_prod and the products"""
    for i in range(n):
        a = rfloat(rng, F64, 997, 1010)
        yield "q_split_f64", (a,)
        thresh = 6.69692879491417e+299                              # the header's literal, as a double
        yield "q_split_f64", (rng.choice((-1, 1)) * rng.choice((thresh, nextup(F64, thresh), math.ldexp(1.0, 996))),)
        yield "q_two_prod_f64", (a, rfloat(rng, F64, -1000, -990))
        q = rq4(rng, F64, rng.randint(997, 1005), 4)
        yield "q_mul_scalar_f64", (q, rfloat(rng, F64, -1000, -995))
        if i % 4 == 0:
            yield "q_mul_f64", (q, rq4(rng, F64, rng.randint(-860, -850), 4))


def g_q4_float_underflow(rng, n):
    """q4<float> operands whose low words underflow: subnormal and flushed-to-zero last words"""
    for i in range(n):
        e0 = rng.randint(-75, -50)
        a = tuple(r32(x) for x in rq4(rng, F32, e0, 4))          # the low words become subnormals or zeros
        b = rq4(rng, F32, rng.randint(-10, 10), 4)
        yield "q_add_f32", (a, tuple(r32(x) for x in rq4(rng, F32, e0 + rng.randint(-3, 3), 4)))
        yield "q_mul_scalar_f32", (a, b[0])
        yield "q_mul_pwr2_f32", (a, math.ldexp(1.0, -rng.randint(1, 30)))
        if i % 4 == 0:
            yield "q_mul_f32", (a, b)
            yield "q_sqr_f32", (rq4(rng, F32, rng.randint(-40, -25), 4),)


def g_add2(rng, n):
    """the eleven boundary gaps as hr_add2<false> / hr_add2<true> cases (x and y draw their gap independently), with equal,
    opposite, nearly opposite and unrelated mantissas"""
    D = Draw(RDF, rng)
    for _ in range(n):
        for gx in GAPS:
            for rel in ("equal", "opposite", "nearly_opposite", "unrelated"):
                gy = rng.choice(GAPS)
                ops = []
                for g in (gx, gy):
                    am = D.norm()
                    s = g if abs(g) < 120 else 0
                    bm = {"equal": D.scale(am, s), "opposite": D.neg(D.scale(am, s)), "nearly_opposite": D.neg(D.near(D.scale(am, s))),
                          "unrelated": D.unnorm(3)}[rel]
                    base = rng.randint(-3000, 3000)
                    ops.append(((am, base + g), (bm, base)))
                a, b = (ops[0][0], ops[1][0]), (ops[0][1], ops[1][1])
                yield "hr_add2_add", (a, b)
                yield "hr_add2_sub", (a, b)
    # whole waves (64 consecutive cases) in which both gaps of every lane are 120 or more: the wave-uniform early return
    for op in ("hr_add2_add", "hr_add2_sub"):
        for _ in range(128):
            yield op, (((D.norm(), 500), (D.norm(), 700)), ((D.unnorm(3), 500 - rng.choice((120, 121, 130, 4000))),
                                                          (D.unnorm(3), 700 - rng.choice((120, 121, 130, 4000)))))


def g_add2_random(rng, n):
    """hr_add2 between the boundaries: gaps drawn from -125 .. 125, mantissas over a few binades, zero tails now and then"""
    D = Draw(RDF, rng)
    for _ in range(n):
        a, b = [], []
        for _part in range(2):
            g, base = rng.randint(-125, 125), rng.randint(-3000, 3000)
            a.append((D.unnorm(3), base + g))
            b.append((D.unnorm(3), base))
        yield rng.choice(("hr_add2_add", "hr_add2_sub")), (tuple(a), tuple(b))


# ------------------------------------------------------------------------------------------------ families
class Case:
    __slots__ = ("op", "cls", "args", "out", "in_words", "out_words")


class Family:
    def __init__(self, name, gens):
        self.name, self.gens = name, gens
        self.cases, self.draws, self.redraws, self.arms = None, 0, 0, None


def _hdr_gens(T, S, seed, scale=1):
    mk = lambda g, n, k: (g.__name__[2:], lambda: g(T, S, random.Random(seed + k), n))
    gens = [mk(g_gaps, 1 * scale, 1), mk(g_zero_mantissa, 1, 2), mk(g_exp_cross, 6, 3), mk(g_square_wrap, 3, 4),
            mk(g_mantissas, 40 * scale, 5), mk(g_compare, 12, 6), mk(g_multiplier, 60, 7), mk(g_subnormal_products, 6, 8),
            mk(g_reduce, 8, 9)]
    if T is not RDF:
        gens.append(mk(g_div_sqrt, 40, 10))
    return gens


def _dw_gens(prefix, fmt, S, seed, ops_add, ops_mul, n):
    return [("pairs", lambda: g_dw_pairs(prefix, fmt, S, random.Random(seed + 1), n, ops_add + ops_mul)),
            ("cancellation", lambda: g_dw_cancel(prefix, fmt, S, random.Random(seed + 2), n // 2, ops_add)),
            ("exact_products", lambda: g_dw_exact_products(prefix, fmt, S, random.Random(seed + 3), n // 2, ops_mul))]


def _two_sum_gen(fmt, S, seed, n):
    def g():
        rng = random.Random(seed)
        for _ in range(n):
            a, b = rfloat(rng, fmt, -60, 60), rfloat(rng, fmt, -60, 60)
            for x, y in ((a, b), (a, -a), (a, 0.0), (-0.0, 0.0), (a, math.ldexp(b, -fmt.p - 2)), (rsub(rng, fmt), rsub(rng, fmt))):
                yield "dw_two_sum_" + S, (x, y)
            h = rdw(rng, fmt, -60, 60)
            yield "dw_sqr_" + S, (h,)
            yield "dw_sqr_" + S, ((math.ldexp(rng.getrandbits(fmt.p // 2 - 1) | 1, rng.randint(-30, 30)), 0.0),)
    return ("two_sum_and_squares", g)


def _fma_gens(seed, n):
    def run(cls):
        def g():
            for c, args in g_fma_down(random.Random(seed), n):
                if c == cls:
                    yield "fma_down_f32", args
        return g
    return [(c, run(c)) for c in ("exact", "exact_zero_sum", "just_off_representable", "tie", "random", "subnormal")]


FAMILIES = {f.name: f for f in (
    Family("hdr_f32", _hdr_gens(R32, "f32", 1000)),
    Family("hdr_f64", _hdr_gens(R64, "f64", 2000)),
    Family("hdr_df32", _hdr_gens(RDF, "df32", 3000)),
    Family("df32", _dw_gens("df32_", F32, "", 4000, ["add", "sub"], ["mul"], 300) +
           [("compare", lambda: g_df32_compare(random.Random(4010), 40))]),
    Family("qd_f32", [("expansions", lambda: g_q4(F32, "f32", random.Random(5001), 120, 1)),
                      ("pieces", lambda: g_q4_pieces(F32, "f32", random.Random(5002), 60)),
                      ("low_words_underflow", lambda: g_q4_float_underflow(random.Random(5003), 80))]),
    Family("qd_f64", [("expansions", lambda: g_q4(F64, "f64", random.Random(6001), 120, 1)),
                      ("pieces", lambda: g_q4_pieces(F64, "f64", random.Random(6002), 60)),
                      ("heads_above_2^996", lambda: g_q4_double_high(random.Random(6003), 40))]),
    Family("bla", [("bla_f32", lambda: g_bla(R32, "f32", random.Random(7001), 25)),
                   ("bla_f64", lambda: g_bla(R64, "f64", random.Random(7002), 25))]),
    Family("dw", _dw_gens("dw_", F32, "_f32", 8000, ["add", "sub"], ["mul", "mul2x"], 200) +
           _dw_gens("dw_", F64, "_f64", 8100, ["add", "sub"], ["mul"], 200) +
           [_two_sum_gen(F32, "f32", 8200, 60), _two_sum_gen(F64, "f64", 8300, 60)]),
    Family("fma_down", _fma_gens(9000, 150)),
    Family("hr_add2", [("boundary_gaps", lambda: g_add2(random.Random(10000), 3)),
                       ("random_gaps", lambda: g_add2_random(random.Random(10001), 300))]),
)}

MAX_TRIES = 50


def build(name):
    """the cases of a family, each with its model result (cached); fills .draws, .redraws and .arms (the model arms reached)"""
    fam = FAMILIES[name]
    if fam.cases is not None:
        return fam.cases
    saved, M.ARMS = M.ARMS, {}
    cases = []
    try:
        for cls, gen in fam.gens:
            for opname, args in gen():
                fam.draws += 1
                op = OPS[opname]
                before = dict(M.ARMS)
                M.STATE.nonfinite = False
                out = op.fn(*args)
                if M.STATE.nonfinite:
                    # a non-finite intermediate: the draw is dropped (counted), the arms it reached with it
                    fam.redraws += 1
                    M.ARMS = before
                    continue
                c = Case()
                c.op, c.cls, c.args, c.out = op, cls, args, out
                w = []
                for t, v in zip(op.ins, args):
                    pack(t, v, w)
                assert len(w) == op.words_in <= IN_WORDS, opname
                c.in_words = w + [0] * (IN_WORDS - len(w))
                c.out_words = pack(op.out, out, [])
                assert len(c.out_words) == op.words_out <= OUT_WORDS
                cases.append(c)
        fam.arms = M.ARMS
    finally:
        M.ARMS = saved
    # stable by id: arith_device makes one launch per contiguous run of a family's ids
    cases.sort(key=lambda c: c.op.id)
    fam.cases = cases
    return cases


def all_cases():
    """every family's cases in one list sorted by op id, and the slice of each family's cases in it"""
    rows = []
    for name in FAMILIES:
        for c in build(name):
            rows.append((c.op.id, len(rows), name, c))
    rows.sort(key=lambda r: (r[0], r[1]))
    where = {name: [] for name in FAMILIES}
    for i, (_, _, name, c) in enumerate(rows):
        where[name].append(i)
    return [r[3] for r in rows], where


def write_case_file(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<17I", c.op.id, *c.in_words))


def read_out_file(path, n):
    data = open(path, "rb").read()
    assert len(data) == n * OUT_WORDS * 4, (len(data), n)
    w = struct.unpack("<%dI" % (n * OUT_WORDS), data)
    return [w[i * OUT_WORDS:(i + 1) * OUT_WORDS] for i in range(n)]
