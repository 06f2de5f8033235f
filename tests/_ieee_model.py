"""An exact model of the arithmetic headers (csrc/hdr_math.hpp, df32_math.hpp, qd_math.hpp, bla_math.hpp, dw_math.hpp), standard
library only.

The base is ONE IEEE-754 operation: the exact rational result (held as integer numerator / denominator times a power of two) rounded
once, to nearest-even, into binary32 or binary64 -- subnormals, overflow to infinity and the sign of zero by the standard's rules.
fma_down is the fused multiply-add rounded toward minus infinity.  A binary32 / binary64 value is carried as a Python float (every
binary32 value is one), so -0.0 and the infinities are themselves.

On top of it every header function is restated step by step from what its comments document and from the published algorithms
(Knuth two-sum, Dekker split / product, the Hida-Li-Bailey renormalisation).  Nothing here imports the product.

Branching functions call arm(function, arm-name); ARMS collects what a run reached.  An operation that meets or makes a non-finite
value sets STATE.nonfinite (the case generators redraw such cases).
"""
import math
import struct

KMIN = -268435456          # kMinBigExp
GAP = 120                  # kExpDiffIgnored


class _State:
    nonfinite = False


STATE = _State()
ARMS = {}


def arm(fn, name):
    k = (fn, name)
    ARMS[k] = ARMS.get(k, 0) + 1


def wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


# ------------------------------------------------------------------------------------------------ one IEEE operation
class Fmt:
    def __init__(self, name, p, emax, code, icode, nbits):
        self.name, self.p, self.emax, self.emin = name, p, emax, 1 - emax
        self.code, self.icode, self.nbits = code, icode, nbits
        self.bias = emax
        self.shift = p - 1
        self.expmask = ((1 << (nbits - p)) - 1) << self.shift
        self.keepmask = ((1 << nbits) - 1) ^ self.expmask
        self.oneexp = self.bias << self.shift
        self.max = math.ldexp((1 << p) - 1, emax - p + 1)
        self.tiny = math.ldexp(1.0, self.emin - p + 1)      # smallest subnormal
        self.minnorm = math.ldexp(1.0, self.emin)

    def bits(self, x):
        return struct.unpack(self.icode, struct.pack(self.code, x))[0]

    def from_bits(self, u):
        return struct.unpack(self.code, struct.pack(self.icode, u))[0]

    def __repr__(self):
        return self.name


F32 = Fmt("f32", 24, 127, "<f", "<I", 32)
F64 = Fmt("f64", 53, 1023, "<d", "<Q", 64)
_TWO53 = 9007199254740992.0


def _dec(x):
    """finite float -> (M, E), x = M * 2^E exactly"""
    m, e = math.frexp(x)
    return int(m * _TWO53), e - 53


def _finite(*xs):
    for x in xs:
        if x != x or x in (math.inf, -math.inf):
            STATE.nonfinite = True
            return False
    return True


def _rnd(fmt, N, D, E, down=False):
    """N / D * 2^E (N a non-zero integer, D > 0) rounded once into fmt"""
    neg = N < 0
    n = -N if neg else N
    e = n.bit_length() - D.bit_length()
    if (n < (D << e)) if e >= 0 else ((n << -e) < D):
        e -= 1
    e += E                                   # 2^e <= |value| < 2^(e+1)
    if e < fmt.emin:
        e = fmt.emin                         # subnormal range: fixed quantum
    q = e - fmt.p + 1
    sh = E - q
    if sh >= 0:
        num, den = n << sh, D
    else:
        num, den = n, D << -sh
    m, r = divmod(num, den)
    if down:
        up = neg and r != 0
    else:
        up = 2 * r > den or (2 * r == den and (m & 1))
    if up:
        m += 1
    if m.bit_length() + q - 1 > fmt.emax:    # overflow
        STATE.nonfinite = True
        if down and not neg:
            return fmt.max
        return -math.inf if neg else math.inf
    v = math.ldexp(m, q)
    return -v if neg else v


def _neg0(x):
    return math.copysign(1.0, x) < 0


def _zero_sum(sa, sb, down):
    """sign rule for an exactly zero sum of terms with signs sa, sb (True = negative)"""
    if sa == sb:
        return -0.0 if sa else 0.0
    return -0.0 if down else 0.0


def add(fmt, a, b, down=False):
    if not _finite(a, b):
        return a + b
    (ma, ea), (mb, eb) = _dec(a), _dec(b)
    E = min(ea, eb)
    N = (ma << (ea - E)) + (mb << (eb - E))
    if N == 0:
        if a == 0 and b == 0:
            return _zero_sum(_neg0(a), _neg0(b), down)
        return -0.0 if down else 0.0
    return _rnd(fmt, N, 1, E, down)


def sub(fmt, a, b):
    return add(fmt, a, -b)


def mul(fmt, a, b):
    if not _finite(a, b):
        return a * b
    (ma, ea), (mb, eb) = _dec(a), _dec(b)
    N = ma * mb
    if N == 0:
        return -0.0 if _neg0(a) != _neg0(b) else 0.0
    return _rnd(fmt, N, 1, ea + eb)


def div(fmt, a, b):
    if not _finite(a, b) or b == 0:
        STATE.nonfinite = True
        return math.nan
    (ma, ea), (mb, eb) = _dec(a), _dec(b)
    if ma == 0:
        return -0.0 if _neg0(a) != _neg0(b) else 0.0
    if mb < 0:
        ma, mb = -ma, -mb
    return _rnd(fmt, ma, mb, ea - eb)


def sqrt(fmt, a):
    if not _finite(a) or (a < 0):
        STATE.nonfinite = True
        return math.nan
    if a == 0:
        return a
    m, e = _dec(a)
    k = 64                                   # 2 * 64 extra bits: the root has more than p + 2 bits
    if (e - 2 * k) & 1:
        m <<= 1
        e -= 1
    N = m << (2 * k)
    s = math.isqrt(N)
    # a root of a float is never a rounding tie, so a sticky half unit below the last bit decides every case
    n2 = 2 * s + (1 if s * s != N else 0)
    return _rnd(fmt, n2, 1, (e - 2 * k) // 2 - 1)


def fma(fmt, a, b, c, down=False):
    if not _finite(a, b, c):
        return a * b + c
    (ma, ea), (mb, eb), (mc, ec) = _dec(a), _dec(b), _dec(c)
    mp, ep = ma * mb, ea + eb
    E = min(ep, ec)
    N = (mp << (ep - E)) + (mc << (ec - E))
    if N == 0:
        if mp == 0 and mc == 0:
            return _zero_sum(_neg0(a) != _neg0(b), _neg0(c), down)
        return -0.0 if down else 0.0
    return _rnd(fmt, N, 1, E, down)


def fma_down(fmt, a, b, c):
    return fma(fmt, a, b, c, down=True)


# ------------------------------------------------------------------------------------------------ numeric types F
class Real:
    """F = float or double"""

    def __init__(self, fmt):
        self.fmt = fmt
        self.name = fmt.name
        self.zero, self.one = 0.0, 1.0

    def add(self, a, b):
        return add(self.fmt, a, b)

    def sub(self, a, b):
        return sub(self.fmt, a, b)

    def mul(self, a, b):
        return mul(self.fmt, a, b)

    def div(self, a, b):
        return div(self.fmt, a, b)

    def sqrt(self, a):
        return sqrt(self.fmt, a)

    def neg(self, a):
        return -a

    def eq0(self, a):
        return a == 0

    def lt(self, a, b):
        return a < b

    def gt(self, a, b):
        return a > b

    def le(self, a, b):
        return a <= b

    def fabs(self, a):
        return math.copysign(a, 1.0)     # the sign bit cleared

    def multiplier(self, s):
        f = self.fmt
        if s <= -f.bias:
            arm("multiplier_" + f.name, "zero")
            return 0.0
        if s >= f.emax + 1:
            arm("multiplier_" + f.name, "type_max")
            return f.max
        arm("multiplier_" + f.name, "pow2")
        return math.ldexp(1.0, s)

    def multiplier_neg(self, s):
        f = self.fmt
        if s <= -f.bias:
            arm("multiplier_neg_" + f.name, "zero")
            return 0.0
        arm("multiplier_neg_" + f.name, "pow2")
        assert s <= f.emax, "multiplier_neg is defined for s <= emax only"
        return math.ldexp(1.0, s)

    def reduce(self, m, e):
        """hr_reduce: mantissa to [1, 2) by its exponent FIELD (a subnormal has field 0 and is mis-normalised on purpose)"""
        f = self.fmt
        if m == 0:
            arm("hr_reduce_" + f.name, "zero_keeps_exponent")
            return m, e
        b = f.bits(m)
        field = (b & f.expmask) >> f.shift
        arm("hr_reduce_" + f.name, "subnormal" if field == 0 else "normal")
        return f.from_bits((b & f.keepmask) | f.oneexp), wrap32(e + field - f.bias)

    def exp_field(self, v):
        f = self.fmt
        return (f.bits(v) & f.expmask) >> f.shift


R32, R64 = Real(F32), Real(F64)


def _dw_add(f, a, b):
    ah, at = a
    bh, bt = b
    t1 = add(f, ah, bh)
    t2 = sub(f, t1, ah)
    t3 = add(f, add(f, ah, sub(f, t2, t1)), sub(f, bh, t2))
    t4 = add(f, at, bt)
    t2 = sub(f, t4, at)
    t5 = add(f, add(f, at, sub(f, t2, t4)), sub(f, bt, t2))
    t3 = add(f, t3, t4)
    t4 = add(f, t1, t3)
    t3 = add(f, sub(f, t1, t4), t3)
    t3 = add(f, t3, t5)
    e = add(f, t4, t3)
    return (e, add(f, sub(f, t4, e), t3))


def _dw_sub(f, a, b):
    ah, at = a
    bh, bt = b
    t1 = sub(f, ah, bh)
    t2 = sub(f, t1, ah)
    t3 = sub(f, add(f, ah, sub(f, t2, t1)), add(f, bh, t2))
    t4 = sub(f, at, bt)
    t2 = sub(f, t4, at)
    t5 = sub(f, add(f, at, sub(f, t2, t4)), add(f, bt, t2))
    t3 = add(f, t3, t4)
    t4 = add(f, t1, t3)
    t3 = add(f, sub(f, t1, t4), t3)
    t3 = add(f, t3, t5)
    e = add(f, t4, t3)
    return (e, add(f, sub(f, t4, e), t3))


def _dw_mul(f, a, b):
    ah, at = a
    bh, bt = b
    th = mul(f, ah, bh)
    tt = fma(f, ah, bh, -th)
    tt = fma(f, at, bt, tt)
    tt = fma(f, ah, bt, tt)
    tt = fma(f, at, bh, tt)
    e = add(f, th, tt)
    return (e, add(f, sub(f, th, e), tt))


class DF:
    """F = df32: (head, tail) of binary32"""
    name = "df32"
    fmt = F32
    zero, one = (0.0, 0.0), (1.0, 0.0)

    def add(self, a, b):
        return _dw_add(F32, a, b)

    def sub(self, a, b):
        return _dw_sub(F32, a, b)

    def mul(self, a, b):
        return _dw_mul(F32, a, b)

    def neg(self, a):
        return (-a[0], -a[1])

    def lt(self, a, b):
        return a[0] < b[0] or (a[0] == b[0] and a[1] < b[1])

    def eq(self, a, b):
        return a[0] == b[0] and a[1] == b[1]

    def gt(self, a, b):
        return not self.lt(a, b) and not self.eq(b, a)

    def ge(self, a, b):
        return not self.lt(a, b)

    def le(self, a, b):
        return not self.gt(b, a)

    def eq0(self, a):
        return self.eq(a, self.zero)

    def fabs(self, a):
        if self.lt(a, self.zero):
            arm("fabs_bits_df32", "negated")
            return self.neg(a)
        arm("fabs_bits_df32", "kept")
        return a

    def multiplier(self, s):
        if s <= -127 or s >= 128:
            arm("multiplier_df32", "zero_low" if s <= -127 else "zero_high")
            return (0.0, 0.0)
        arm("multiplier_df32", "pow2")
        return (math.ldexp(1.0, s), 0.0)

    def multiplier_neg(self, s):
        if s <= -127:
            arm("multiplier_neg_df32", "zero")
            return (0.0, 0.0)
        arm("multiplier_neg_df32", "pow2")
        assert s <= 127
        return (math.ldexp(1.0, s), 0.0)

    def reduce(self, m, e):
        """hr_reduce<df32>: the head to [1, 2); the tail's exponent FIELD shifted by the same amount, saturating at field 0"""
        h, t = m
        if h == 0 and t == 0:
            arm("hr_reduce_df32", "zero_keeps_exponent")
            return m, e
        by, bx = F32.bits(h), F32.bits(t)
        fy = ((by & 0x7F800000) >> 23) - 127
        fx = (bx & 0x7F800000) >> 23
        ne = fx - fy
        if ne <= 0:
            arm("hr_reduce_df32", "tail_saturates")
            se = 0
        else:
            arm("hr_reduce_df32", "tail_shifted")
            se = ne
        # (a field above 255 cannot be kept in 8 bits: the generators stay below it, as the product's callers do)
        assert se <= 255
        return (F32.from_bits((by & 0x807FFFFF) | 0x3F800000), F32.from_bits((bx & 0x807FFFFF) | (se << 23))), wrap32(e + fy)


RDF = DF()


# ------------------------------------------------------------------------------------------------ hdr_math.hpp
def clamp_exp(e):
    e = wrap32(e)
    if e < KMIN:
        arm("clamp_exp", "clamped")
        return KMIN
    arm("clamp_exp", "kept")
    return e


def hr_reduce(T, a):
    return T.reduce(a[0], a[1])


def hr_from_mant(T, v):
    return T.reduce(v, 0)


def hr_from_number(T, v):
    f = T.fmt
    if v == 0:
        arm("hr_from_number_" + f.name, "zero")
        return (0.0, KMIN)
    arm("hr_from_number_" + f.name, "nonzero")
    b = f.bits(v)
    return (f.from_bits((b & f.keepmask) | f.oneexp), ((b & f.expmask) >> f.shift) - f.bias)


def hr_mul(T, a, b):
    return (T.mul(a[0], b[0]), clamp_exp(a[1] + b[1]))


def hr_mul2(T, a):
    return (T.mul(a[0], T.one), clamp_exp(a[1] + 1))


def hr_div(T, a, b):
    return (T.div(a[0], b[0]), clamp_exp(a[1] - b[1]))


def hr_square(T, a):
    return (T.mul(a[0], a[0]), wrap32(a[1] * 2))


def _hr_addsub(T, a, b, minus, fn):
    am, ae = a
    bm, be = b
    op = T.sub if minus else T.add
    d = wrap32(ae - be)
    key = fn + "_" + T.name
    if d >= GAP:
        arm(key, "a_dominates_early_return")
        return a
    if d >= 0:
        arm(key, "scale_b")
        am = op(am, T.mul(bm, T.multiplier_neg(-d)))
    elif d > -GAP:
        arm(key, "scale_a")
        ae = be
        am = op(T.mul(am, T.multiplier_neg(d)), bm)
    else:
        arm(key, "b_dominates")
        ae = be
        am = T.neg(bm) if minus else bm
    if T.eq0(am):
        arm(key, "zero_resets_exponent")
        ae = KMIN
    return (am, ae)


def hr_add(T, a, b):
    return _hr_addsub(T, a, b, False, "hr_add")


def hr_sub(T, a, b):
    return _hr_addsub(T, a, b, True, "hr_sub")


def hr_recip(T, a):
    return (T.div(1.0, a[0]), wrap32(-a[1]))


def hr_abs(T, a):
    return (T.fabs(a[0]), a[1])


def hr_cmp_pos(T, a, b):
    if a[1] > b[1]:
        return 1
    if a[1] < b[1]:
        return -1
    if T.gt(a[0], b[0]):
        return 1
    if T.lt(a[0], b[0]):
        return -1
    return 0


def hr_cmp(T, a, b):
    if T.eq0(a[0]) and T.eq0(b[0]):
        return 0
    z = T.zero
    m3 = lambda: 1 if T.gt(a[0], b[0]) else (-1 if T.lt(a[0], b[0]) else 0)
    if T.gt(a[0], z):
        if T.le(b[0], z):
            return 1
        if a[1] > b[1]:
            return 1
        if a[1] < b[1]:
            return -1
        return m3()
    if T.gt(b[0], z):
        return -1
    if a[1] > b[1]:
        return -1
    if a[1] < b[1]:
        return 1
    return m3()


def hr_max_pos(T, a, b):
    return a if hr_cmp_pos(T, a, b) > 0 else b


def hr_min_pos(T, a, b):
    return a if hr_cmp_pos(T, a, b) < 0 else b


def hr_to_native(T, a):
    return T.mul(a[0], T.multiplier(a[1]))


def hc_from_hr(T, re, im):
    e = max(re[1], im[1])
    return (T.mul(re[0], T.multiplier(wrap32(re[1] - e))), T.mul(im[0], T.multiplier(wrap32(im[1] - e))), e)


def hc_from_native(T, re, im):
    return hc_from_hr(T, hr_from_mant(T, re), hr_from_mant(T, im))


def hc_add(T, a, b):
    are, aim, ae = a
    bre, bim, be = b
    d = wrap32(ae - be)
    key = "hc_add_" + T.name
    if d >= GAP:
        arm(key, "a_dominates_early_return")
        return a
    if d >= 0:
        arm(key, "scale_b")
        m = T.multiplier(-d)
        return (T.add(are, T.mul(bre, m)), T.add(aim, T.mul(bim, m)), ae)
    if d > -GAP:
        arm(key, "scale_a")
        m = T.multiplier(d)
        return (T.add(T.mul(are, m), bre), T.add(T.mul(aim, m), bim), be)
    arm(key, "b_dominates")
    return b


def hc_add_real(T, a, r):
    are, aim, ae = a
    rm, rexp = r
    d = wrap32(ae - rexp)
    key = "hc_add_real_" + T.name
    if d >= GAP:
        arm(key, "a_dominates_early_return")
        return a
    if d >= 0:
        arm(key, "scale_b")
        return (T.add(are, T.mul(rm, T.multiplier(-d))), aim, ae)
    if d > -GAP:
        arm(key, "scale_a")
        m = T.multiplier(d)
        return (T.add(T.mul(are, m), rm), T.mul(aim, m), rexp)
    arm(key, "b_dominates")
    return (rm, T.zero, rexp)


def hc_mul(T, a, b):
    re = T.sub(T.mul(a[0], b[0]), T.mul(a[1], b[1]))
    im = T.add(T.mul(a[0], b[1]), T.mul(a[1], b[0]))
    return (re, im, clamp_exp(a[2] + b[2]))


def hc_mul_real(T, a, s):
    return (T.mul(a[0], s[0]), T.mul(a[1], s[0]), clamp_exp(a[2] + s[1]))


def hc_mul2(T, a):
    return (T.mul(a[0], T.one), T.mul(a[1], T.one), clamp_exp(a[2] + 1))


def hc_reduce(T, a):
    re, im, e = a
    if T is RDF:
        if T.eq0(re) and T.eq0(im):
            arm("hc_reduce_df32", "zero_keeps_exponent")
            return a
        arm("hc_reduce_df32", "reduced")
        r = hc_from_hr(T, T.reduce(re, 0), T.reduce(im, 0))
        return (r[0], r[1], wrap32(r[2] + e))
    key = "hc_reduce_" + T.name
    if re == 0 and im == 0:
        arm(key, "zero_keeps_exponent")
        return a
    fr, fi = T.exp_field(re), T.exp_field(im)
    arm(key, "both_subnormal_or_zero" if max(fr, fi) == 0 else "reduced")
    d = max(fr, fi) - T.fmt.bias
    m = T.multiplier(-d)
    return (T.mul(re, m), T.mul(im, m), wrap32(e + d))


def hc_norm2(T, a):
    return (T.add(T.mul(a[0], a[0]), T.mul(a[1], a[1])), wrap32(a[2] << 1))


def hc_cheb(T, a):
    ar, ai = T.fabs(a[0]), T.fabs(a[1])
    return (ar if T.gt(ar, ai) else ai, a[2])


def hc_norm(T, a):
    return (T.sqrt(T.add(T.mul(a[0], a[0]), T.mul(a[1], a[1]))), a[2])


def hc_div(T, a, b):
    t = T.div(1.0, T.add(T.mul(b[0], b[0]), T.mul(b[1], b[1])))
    re = T.mul(T.add(T.mul(a[0], b[0]), T.mul(a[1], b[1])), t)
    im = T.mul(T.sub(T.mul(a[1], b[0]), T.mul(a[0], b[1])), t)
    return (re, im, clamp_exp(a[2] - b[2]))


def hc_recip(T, a):
    t = T.div(1.0, T.add(T.mul(a[0], a[0]), T.mul(a[1], a[1])))
    return (T.mul(a[0], t), T.mul(-a[1], t), wrap32(-a[2]))


def hr2_from_float(v):
    if v == 0:
        arm("hr2_from_float", "zero")
        return ((0.0, 0.0), KMIN)
    arm("hr2_from_float", "nonzero")
    b = F32.bits(v)
    return ((F32.from_bits((b & 0x807FFFFF) | 0x3F800000), 0.0), ((b & 0x7F800000) >> 23) - 127)


# ------------------------------------------------------------------------------------------------ bla_math.hpp
def bla_sqrt(T, a):
    m, e = a
    if e & 1:
        arm("bla_sqrt_" + T.name, "odd_exponent")
        return (T.sqrt(T.mul(2.0, m)), (e - 1) // 2)
    arm("bla_sqrt_" + T.name, "even_exponent")
    return (T.sqrt(m), e // 2)


def bla_hypot(T, a, b):
    return hr_reduce(T, bla_sqrt(T, hr_add(T, hr_mul(T, a, a), hr_mul(T, b, b))))


# ------------------------------------------------------------------------------------------------ dw_math.hpp
def dw_two_sum(f, a, b):
    h = add(f, a, b)
    t1 = sub(f, h, a)
    t2 = sub(f, h, t1)
    t1 = sub(f, b, t1)
    t2 = sub(f, a, t2)
    return (h, add(f, t1, t2))


dw_add, dw_sub, dw_mul = _dw_add, _dw_sub, _dw_mul


def dw_mul2x(f, a, b):
    h, t = _dw_mul(f, a, b)
    return (mul(f, h, 2.0), mul(f, t, 2.0))


def dw_sqr(f, a):
    h, t = a
    th = mul(f, h, h)
    tt = fma(f, h, h, -th)
    tt = fma(f, t, t, tt)
    if f is F32:
        tt = fma(f, 2.0, mul(f, h, t), tt)       # the cross term as one product doubled inside an fma
    else:
        tt = fma(f, h, t, tt)                    # the cross term as two fmas
        tt = fma(f, t, h, tt)
    e = add(f, th, tt)
    return (e, add(f, sub(f, th, e), tt))


# ------------------------------------------------------------------------------------------------ qd_math.hpp
def _zs(f):
    return f is F64            # zero shortcuts: QuadDouble only


def q_quick_two_sum(f, a, b):
    if _zs(f) and b == 0:
        arm("q_quick_two_sum_" + f.name, "zero_shortcut")
        return add(f, a, b), 0.0
    arm("q_quick_two_sum_" + f.name, "full")
    s = add(f, a, b)
    return s, sub(f, b, sub(f, s, a))


def q_two_sum(f, a, b):
    if _zs(f) and (a == 0 or b == 0):
        arm("q_two_sum_" + f.name, "zero_shortcut")
        return add(f, a, b), 0.0
    arm("q_two_sum_" + f.name, "full")
    s = add(f, a, b)
    bb = sub(f, s, a)
    return s, add(f, sub(f, a, sub(f, s, bb)), sub(f, b, bb))


def q_split(f, a):
    if f is F32:
        arm("q_split_f32", "plain")
        t = mul(f, a, 4097.0)
        hi = sub(f, t, sub(f, t, a))
        return hi, sub(f, a, hi)
    thresh = 6.69692879491417e+299
    if a > thresh or a < -thresh:
        arm("q_split_f64", "scaled_above_2^996")
        a = mul(f, a, 3.7252902984619140625e-09)
        t = mul(f, 134217729.0, a)
        hi = sub(f, t, sub(f, t, a))
        lo = sub(f, a, hi)
        return mul(f, hi, 268435456.0), mul(f, lo, 268435456.0)
    arm("q_split_f64", "plain")
    t = mul(f, 134217729.0, a)
    hi = sub(f, t, sub(f, t, a))
    return hi, sub(f, a, hi)


def q_two_prod(f, a, b):
    p = mul(f, a, b)
    ah, al = q_split(f, a)
    bh, bl = q_split(f, b)
    err = add(f, add(f, add(f, sub(f, mul(f, ah, bh), p), mul(f, ah, bl)), mul(f, al, bh)), mul(f, al, bl))
    return p, err


def q_two_sqr(f, a):
    q = mul(f, a, a)
    hi, lo = q_split(f, a)
    err = add(f, add(f, sub(f, mul(f, hi, hi), q), mul(f, mul(f, 2.0, hi), lo)), mul(f, lo, lo))
    return q, err


def _three_sum(f, a, b, c):
    t1, t2 = q_two_sum(f, a, b)
    a, t3 = q_two_sum(f, c, t1)
    b, c = q_two_sum(f, t2, t3)
    return a, b, c


def _three_sum2(f, a, b, c):
    t1, t2 = q_two_sum(f, a, b)
    a, t3 = q_two_sum(f, c, t1)
    return a, add(f, t2, t3), c


def q_renorm(f, c0, c1, c2, c3, c4):
    """five terms into four; returns (c0, c1, c2, c3).  The arm names spell the path through the zero tests (QuadDouble only)."""
    key = "q_renorm_" + f.name
    qts = q_quick_two_sum
    zs = _zs(f)
    s2 = s3 = 0.0
    s0, c4 = qts(f, c3, c4)
    s0, c3 = qts(f, c2, s0)
    s0, c2 = qts(f, c1, s0)
    c0, c1 = qts(f, c0, s0)
    s0, s1 = qts(f, c0, c1)
    if not zs:
        arm(key, "no_zero_tests")
    if not zs or s1 != 0:
        s1, s2 = qts(f, s1, c2)
        if not zs or s2 != 0:
            s2, s3 = qts(f, s2, c3)
            if not zs or s3 != 0:
                if zs:
                    arm(key, "s1!=0,s2!=0,s3!=0")
                s3 = add(f, s3, c4)
            else:
                arm(key, "s1!=0,s2!=0,s3==0")
                s2 = add(f, s2, c4)
        else:
            s1, s2 = qts(f, s1, c3)
            if s2 != 0:
                arm(key, "s1!=0,s2==0,then s2!=0")
                s2, s3 = qts(f, s2, c4)
            else:
                arm(key, "s1!=0,s2==0,then s2==0")
                s1, s2 = qts(f, s1, c4)
    else:
        s0, s1 = qts(f, s0, c2)
        if s1 != 0:
            s1, s2 = qts(f, s1, c3)
            if s2 != 0:
                arm(key, "s1==0,then s1!=0,s2!=0")
                s2, s3 = qts(f, s2, c4)
            else:
                arm(key, "s1==0,then s1!=0,s2==0")
                s1, s2 = qts(f, s1, c4)
        else:
            s0, s1 = qts(f, s0, c3)
            if s1 != 0:
                arm(key, "s1==0,then s1==0,then s1!=0")
                s1, s2 = qts(f, s1, c4)
            else:
                arm(key, "s1==0,then s1==0,then s1==0")
                s0, s1 = qts(f, s0, c4)
    return (s0, s1, s2, s3)


def q_add(f, a, b):
    s = [add(f, a[i], b[i]) for i in range(4)]
    v = [sub(f, s[i], a[i]) for i in range(4)]
    u = [sub(f, s[i], v[i]) for i in range(4)]
    w = [sub(f, a[i], u[i]) for i in range(4)]
    u = [sub(f, b[i], v[i]) for i in range(4)]
    t = [add(f, w[i], u[i]) for i in range(4)]
    s[1], t[0] = q_two_sum(f, s[1], t[0])
    s[2], t[0], t[1] = _three_sum(f, s[2], t[0], t[1])
    s[3], t[0], t[2] = _three_sum2(f, s[3], t[0], t[2])
    t[0] = add(f, add(f, t[0], t[1]), t[3])
    return q_renorm(f, s[0], s[1], s[2], s[3], t[0])


def q_neg(a):
    return tuple(-x for x in a)


def q_sub(f, a, b):
    return q_add(f, a, q_neg(b))


def q_mul_pwr2(f, a, b):
    return tuple(mul(f, x, b) for x in a)


def q_mul_scalar(f, a, b):
    p0, q0 = q_two_prod(f, a[0], b)
    p1, q1 = q_two_prod(f, a[1], b)
    p2, q2 = q_two_prod(f, a[2], b)
    p3 = mul(f, a[3], b)
    s0 = p0
    s1, s2 = q_two_sum(f, q0, p1)
    s2, q1, p2 = _three_sum(f, s2, q1, p2)
    q1, q2, p3 = _three_sum2(f, q1, q2, p3)
    s3 = q1
    s4 = add(f, q2, p2)
    return q_renorm(f, s0, s1, s2, s3, s4)


def q_mul(f, a, b):
    p0, q0 = q_two_prod(f, a[0], b[0])
    p1, q1 = q_two_prod(f, a[0], b[1])
    p2, q2 = q_two_prod(f, a[1], b[0])
    p3, q3 = q_two_prod(f, a[0], b[2])
    p4, q4v = q_two_prod(f, a[1], b[1])
    p5, q5 = q_two_prod(f, a[2], b[0])
    p1, p2, q0 = _three_sum(f, p1, p2, q0)
    p2, q1, q2 = _three_sum(f, p2, q1, q2)
    p3, p4, p5 = _three_sum(f, p3, p4, p5)
    s0, t0 = q_two_sum(f, p2, p3)
    s1, t1 = q_two_sum(f, q1, p4)
    s2 = add(f, q2, p5)
    s1, t0 = q_two_sum(f, s1, t0)
    s2 = add(f, s2, add(f, t0, t1))
    acc = mul(f, a[0], b[3])
    for x, y in ((a[1], b[2]), (a[2], b[1]), (a[3], b[0])):
        acc = add(f, acc, mul(f, x, y))
    for x in (q0, q3, q4v, q5):
        acc = add(f, acc, x)
    s1 = add(f, s1, acc)
    return q_renorm(f, p0, p1, s0, s1, s2)


def q_sqr(f, a):
    p0, q0 = q_two_sqr(f, a[0])
    p1, q1 = q_two_prod(f, mul(f, 2.0, a[0]), a[1])
    p2, q2 = q_two_prod(f, mul(f, 2.0, a[0]), a[2])
    p3, q3 = q_two_sqr(f, a[1])
    p1, q0 = q_two_sum(f, q0, p1)
    q0, q1 = q_two_sum(f, q0, q1)
    p2, p3 = q_two_sum(f, p2, p3)
    s0, t0 = q_two_sum(f, q0, p2)
    s1, t1 = q_two_sum(f, q1, p3)
    s1, t0 = q_two_sum(f, s1, t0)
    t0 = add(f, t0, t1)
    s1, t0 = q_quick_two_sum(f, s1, t0)
    p2, t1 = q_quick_two_sum(f, s0, s1)
    p3, q0 = q_quick_two_sum(f, t1, t0)
    p4 = mul(f, mul(f, 2.0, a[0]), a[3])
    p5 = mul(f, mul(f, 2.0, a[1]), a[2])
    p4, p5 = q_two_sum(f, p4, p5)
    q2, q3 = q_two_sum(f, q2, q3)
    t0, t1 = q_two_sum(f, p4, q2)
    t1 = add(f, add(f, t1, p5), q3)
    p3, p4 = q_two_sum(f, p3, t0)
    p4 = add(f, add(f, p4, q0), t1)
    return q_renorm(f, p0, p1, p2, p3, p4)


def q_le(f, a, b):
    for i in range(3):
        if a[i] < b[i]:
            arm("q_le_" + f.name, "decided_less_at_word_%d" % i)
            return 1
        if a[i] != b[i]:
            arm("q_le_" + f.name, "decided_greater_at_word_%d" % i)
            return 0
    arm("q_le_" + f.name, "decided_at_last_word")
    return 1 if a[3] <= b[3] else 0


def q_le_scalar(f, a, b):
    if a[0] < b:
        arm("q_le_scalar_" + f.name, "head_less")
        return 1
    if a[0] == b:
        arm("q_le_scalar_" + f.name, "head_equal_y_decides")
        return 1 if a[1] <= 0 else 0
    arm("q_le_scalar_" + f.name, "head_greater")
    return 0
