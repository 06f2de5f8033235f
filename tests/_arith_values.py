"""Value checks of the arithmetic-edge tests: the exact rational value of a result against the exact rational result of the
mathematical operation.  They look at result words only (whoever produced them), so they do not depend on tests/_ieee_model.py
being a faithful transcription of the headers.

bound(case) gives, for the functions with a derived bound, (|result - exact|, allowed) as Fractions, or None where the case is out
of the bound's scope (a clamped or wrapped exponent, an arm that drops an operand, an intermediate in the subnormal range where the
derivation says so).  relerr(case, words) gives the relative error of the double-word / expansion results."""
from fractions import Fraction as Fr

from _ieee_model import F32, F64, KMIN, GAP

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def pow2(e):
    return Fr(1 << e) if e >= 0 else Fr(1, 1 << -e)


def unpack(t, w, i=0):
    """result words -> (value, next index); the inverse of _arith_cases.pack"""
    if t in "ib":
        v = w[i]
        return (v - (1 << 32) if (t == "i" and v >> 31) else v), i + 1
    if t == "f":
        return F32.from_bits(w[i]), i + 1
    if t == "d":
        return F64.from_bits(w[i] | (w[i + 1] << 32)), i + 2
    if t == "D":
        parts = ("f", "f")
    elif t[0] == "h":
        parts = (t[1], "i")
    elif t[0] == "c":
        parts = (t[1], t[1], "i")
    elif t[0] == "q":
        parts = (t[1],) * 4
    elif t[0] == "p":
        parts = (t[1],) * 2
    elif t == "A":
        parts = ("hD", "hD", "b")
    else:
        raise ValueError(t)
    out = []
    for p in parts:
        v, i = unpack(p, w, i)
        out.append(v)
    return tuple(out), i


def val(x):
    """exact value of a float, a double-float / double-word pair or an expansion"""
    if isinstance(x, tuple):
        return sum((Fr(v) for v in x), Fr(0))
    return Fr(x)


# ------------------------------------------------------------------------------------------------ hreal / hcplx, F = float | double
# Notation: u = 2^-p is the unit roundoff of F (round to nearest: fl(x) = x (1 + e), |e| <= u, for x in the normal range), t =
# the smallest subnormal (a rounding that lands in the subnormal range errs by at most t / 2 instead).  A sum never underflows
# inexactly (a sum of two floats in the subnormal range is exact), a product or quotient can.
def bound(case, words):
    name = case.op.name
    if not name.endswith(("_f32", "_f64")):
        return None
    fmt = F32 if name.endswith("_f32") else F64
    fn = name[:-4]
    u, t = pow2(-fmt.p), Fr(fmt.tiny)
    res, _ = unpack(case.op.out, words)
    a = case.args[0]
    b = case.args[1] if len(case.args) > 1 else None
    in32 = lambda e: INT_MIN <= e <= INT_MAX

    if fn in ("hr_mul", "hr_div", "hr_square", "hr_recip", "hr_mul2"):
        # ONE rounding of the mantissa product / quotient; the exponent is an exact integer sum unless it is clamped at kMinBigExp
        # (hr_mul, hr_div, hr_mul2) or wraps (hr_square, hr_recip of INT_MIN): out of scope then.
        # |m_res - m_exact| <= max(u |m_exact|, t / 2)
        if fn == "hr_mul":
            m, e = Fr(a[0]) * Fr(b[0]), a[1] + b[1]
        elif fn == "hr_mul2":
            m, e = Fr(a[0]), a[1] + 1
        elif fn == "hr_square":
            m, e = Fr(a[0]) ** 2, 2 * a[1]
        elif fn == "hr_div":
            if b[0] == 0:
                return None
            m, e = Fr(a[0]) / Fr(b[0]), a[1] - b[1]
        else:
            if a[0] == 0:
                return None
            m, e = 1 / Fr(a[0]), -a[1]
        if e < KMIN or not in32(e) or res[1] != e:
            return None if (e < KMIN or not in32(e)) else (Fr(1), Fr(0))
        return abs(Fr(res[0]) - m), max(u * abs(m), t / 2)

    if fn in ("hr_add", "hr_sub"):
        # |gap| < 120: the operand with the smaller exponent is scaled by a power of two (exact, or within t / 2 where it lands in
        # the subnormal range), then ONE rounding of the sum: with s the scaled operand as computed,
        #   m_res = (x + s)(1 + e),  |s - s_exact| <= t / 2   =>   |m_res - (x + s_exact)| <= u |x + s_exact| + (1 + u) t / 2
        # under the larger exponent.  A zero result resets the exponent (the value is still zero).  Gaps of 120 and more drop an
        # operand: out of scope.
        d = a[1] - b[1]
        if abs(d) >= GAP or not in32(d):
            return None
        sg = -1 if fn == "hr_sub" else 1
        E = max(a[1], b[1])
        m = Fr(a[0]) * pow2(a[1] - E) + sg * Fr(b[0]) * pow2(b[1] - E)
        if res[0] == 0:
            return abs(m), (1 + u) * t / 2
        if res[1] != E:
            return Fr(1), Fr(0)
        return abs(Fr(res[0]) - m), u * abs(m) + (1 + u) * t / 2

    if fn in ("hc_mul", "hc_norm2"):
        # each part is fl(fl(p1) +- fl(p2)): THREE roundings.  With A = |p1| + |p2| (no cancellation is assumed: the bound is
        # against the sum of magnitudes), |fl(pi) - pi| <= max(u |pi|, t / 2), and the sum adds u |fl(p1) +- fl(p2)|:
        #   |err| <= u A + t + u (A (1 + u) + t)  =  (2 u + u^2) A + (1 + u) t
        if fn == "hc_mul":
            e = a[2] + b[2]
            if e < KMIN or res[2] != e:
                return None if e < KMIN else (Fr(1), Fr(0))
            ar, ai, br, bi = (Fr(v) for v in (a[0], a[1], b[0], b[1]))
            parts = ((ar * br - ai * bi, abs(ar * br) + abs(ai * bi), res[0]), (ar * bi + ai * br, abs(ar * bi) + abs(ai * br), res[1]))
        else:
            if not in32(2 * a[2]) or res[1] != 2 * a[2]:
                return None if not in32(2 * a[2]) else (Fr(1), Fr(0))
            ar, ai = Fr(a[0]), Fr(a[1])
            parts = ((ar * ar + ai * ai, ar * ar + ai * ai, res[0]),)
        worst = None
        for exact, A, got in parts:
            err, allow = abs(Fr(got) - exact), (2 * u + u * u) * A + (1 + u) * t
            if worst is None or err * worst[1] > worst[0] * allow or (allow == 0 and err > 0):
                worst = (err, allow)
        return worst

    if fn == "hc_mul_real":
        # ONE rounding per part
        e = a[2] + b[1]
        if e < KMIN or res[2] != e:
            return None if e < KMIN else (Fr(1), Fr(0))
        worst = (Fr(0), Fr(1))
        for x, got in ((a[0], res[0]), (a[1], res[1])):
            m = Fr(x) * Fr(b[0])
            err, allow = abs(Fr(got) - m), max(u * abs(m), t / 2)
            if err * worst[1] > worst[0] * allow:
                worst = (err, allow)
        return worst

    if fn in ("hc_norm", "bla_sqrt", "bla_hypot"):
        # the square root of a value n known to a relative error th, rounded once more: sqrt(n (1 + th)) (1 + e), with
        # sqrt(1 + th) <= 1 + th / 2 for th >= 0 and >= 1 + th / 2 - th^2 / 8 ... for th < 0: |rel| <= |th| / 2 + u + (small).
        #   bla_sqrt:  n = m or 2 m exactly (th = 0):                    u
        #   hc_norm:   n = fl(fl(re^2) + fl(im^2)), th <= 2 u + u^2:     2 u + 2 u^2 <= 2.5 u
        #   bla_hypot: the same n through hr_mul, hr_mul and hr_add (equal exponents scale by 1, others by an exact power of two):
        #              2.5 u; hr_reduce afterwards is exact.
        # In scope while no product underflows (every square at least 2^(emin + 1)) and no exponent is clamped.
        if fn == "bla_sqrt":
            n, e, k = Fr(a[0]), a[1], u
            if a[0] < 0:
                return None
        elif fn == "hc_norm":
            n, e, k = Fr(a[0]) ** 2 + Fr(a[1]) ** 2, 2 * a[2], u * 5 / 2
            if any(0 < abs(Fr(v)) ** 2 < 2 * Fr(fmt.minnorm) for v in a[:2]):
                return None
        else:
            if min(2 * a[1], 2 * b[1]) < KMIN or abs(2 * a[1] - 2 * b[1]) >= GAP:
                return None
            E = max(2 * a[1], 2 * b[1])
            sq = [Fr(x[0]) ** 2 * pow2(2 * x[1] - E) for x in (a, b)]
            if any(0 < Fr(x[0]) ** 2 < 2 * Fr(fmt.minnorm) for x in (a, b)) or any(0 < s < 2 * Fr(fmt.minnorm) for s in sq):
                return None
            n, e, k = sq[0] + sq[1], E, u * 5 / 2
        if n == 0:
            return abs(Fr(res[0])), Fr(0)
        # the result r = s 2^es against sqrt(n 2^e), squared to stay rational:
        #   |r - sqrt(N)| <= k sqrt(N)  <=>  (1 - k)^2 N <= r^2 <= (1 + k)^2 N,  with r^2 / N = (s^2 / n) 2^(2 es - e)
        if abs(2 * res[1] - e) > 4200:
            return Fr(1), Fr(0)
        r2 = Fr(res[0]) ** 2 * pow2(2 * res[1] - e)
        ok = (1 - k) ** 2 * n <= r2 <= (1 + k) ** 2 * n
        return (Fr(0), Fr(1)) if ok else (Fr(1), Fr(0))

    if fn in ("hc_div", "hc_recip"):
        # t = fl(1 / n) with n = fl(fl(br^2) + fl(bi^2)) = |b|^2 (1 + th), |th| <= 2 u + u^2, so t = (1 + g) / |b|^2 with
        # |g| <= (1 + u) / (1 - 2 u - u^2) - 1 <= 3 u + 8 u^2; the numerator N is known within (2 u + u^2) A, A its sum of
        # magnitudes (hc_recip: exactly, A = |component|); the last product rounds once more:
        #   |err| <= (A / |b|^2) ((1 + 2 u + u^2)(1 + 3 u + 8 u^2)(1 + u) - 1) <= 7 u A / |b|^2
        # In scope while nothing underflows (every product and the quotient at least 2^(emin + 1), or zero) and no clamp.
        bb = b if fn == "hc_div" else a
        br, bi = Fr(bb[0]), Fr(bb[1])
        n2 = br * br + bi * bi
        if n2 == 0:
            return None
        lim = 2 * Fr(fmt.minnorm)
        if fn == "hc_div":
            e = a[2] - b[2]
            ar, ai = Fr(a[0]), Fr(a[1])
            prods = (ar * br, ai * bi, ai * br, ar * bi)
            parts = ((ar * br + ai * bi, abs(ar * br) + abs(ai * bi), res[0]), (ai * br - ar * bi, abs(ai * br) + abs(ar * bi), res[1]))
        else:
            e = -a[2]
            prods = ()
            parts = ((br, abs(br), res[0]), (-bi, abs(bi), res[1]))
        if e < KMIN or not in32(e):
            return None
        if res[2] != e:
            return Fr(1), Fr(0)
        if any(0 < abs(x) < lim for x in (br * br, bi * bi, 1 / n2) + prods) or any(0 < A / n2 < lim for _, A, _ in parts):
            return None
        worst = (Fr(0), Fr(1))
        for exact, A, got in parts:
            err, allow = abs(Fr(got) - exact / n2), 7 * u * A / n2
            if allow == 0:
                if err:
                    return Fr(1), Fr(0)
                continue
            if err * worst[1] > worst[0] * allow:
                worst = (err, allow)
        return worst
    return None


# ------------------------------------------------------------------------------------------------ df32, dw<T>, q4<T>
# op name -> (the mathematical operation on exact values, the classes it is measured on).  Additions count where the operands have
# the same sign (no cancellation).
_REL = {}
for _n in ("df32_add", "dw_add_f32", "dw_add_f64", "q_add_f32", "q_add_f64"):
    _REL[_n] = "add"
for _n in ("df32_mul", "dw_mul_f32", "dw_mul_f64", "q_mul_f32", "q_mul_f64", "q_mul_scalar_f32", "q_mul_scalar_f64"):
    _REL[_n] = "mul"
for _n in ("dw_sqr_f32", "dw_sqr_f64", "q_sqr_f32", "q_sqr_f64"):
    _REL[_n] = "sqr"
REL_CLASSES = ("pairs", "expansions", "two_sum_and_squares")


def relerr(case, words):
    """relative error of a double-word / expansion sum, product or square against the exact one, or None out of scope"""
    kind = _REL.get(case.op.name)
    if kind is None or case.cls not in REL_CLASSES:
        return None
    res, _ = unpack(case.op.out, words)
    a = val(case.args[0])
    if kind == "sqr":
        exact = a * a
    else:
        b = val(case.args[1])
        if kind == "add":
            if (a > 0) != (b > 0) or a == 0 or b == 0:
                return None
            exact = a + b
        else:
            exact = a * b
    if exact == 0:
        return None
    return abs(val(res) - exact) / abs(exact)
