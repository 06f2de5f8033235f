// exact_math.hpp -- fixed-point Mandelbrot iteration on L 32-bit limbs, for the device (kernels_exact.hip) and for the host
// (g++; tests/exact/exact_host.cpp runs the same functions on the CPU).
//
// The recurrence is the one the project's truth uses (integers only, nothing is ever rounded):
//     x' = floor((x^2 - y^2) / 2^F) + cx        y' = floor(2 x y / 2^F) + cy        escape when x^2 + y^2 > R 2^2F  (>= when inclusive)
// x, y, cx, cy are two's-complement numbers of L limbs, least significant limb first, holding value * 2^F.
//
// How many limbs a frac_bits needs.  Supported: integer 1 <= R <= 256, |cx|, |cy| < 32 * 2^F, 32 L >= F + 10.
//   * A z that has not escaped has x^2 + y^2 <= R 2^2F, so |x|, |y| <= 16 * 2^F and 2|x||y| <= x^2 + y^2 <= 256 * 2^2F.
//   * Its successor: |x'| <= |x^2 - y^2| / 2^F + 1 + |cx| < 256 * 2^F + 1 + 32 * 2^F < 2^(F+9), and |y'| the same way.  z_1 = c is
//     inside that bound too.  So EVERY z this code holds -- the one that fails the escape test included, since it is the successor of
//     one that passed -- is below 2^(F+9) in magnitude and fits F + 10 bits with its sign: L = ceil((F + 10) / 32).
//   * The squares of such values are below 2^(2F+18) and their sum below 2^(2F+19) <= 2^(64L-1): the 2L-limb products, their sum
//     and their difference (as a signed number) never overflow, and R 2^2F < 2^(2F+9) fits 2L limbs as well.
//   * F = 32 q + r with q <= L - 1, so the L + 1 limbs the shift reads (q .. q + L) all lie inside the 2L-limb product.
//
// Multiplication is schoolbook on magnitudes, the signs kept apart: per row, L independent 32 x 32 -> 64 multiply-adds
// (a_i * b_j + p_{i+j} cannot overflow 64 bits), then one carry chain that adds each product's high word into the next column.
// Squares compute the L (L - 1) / 2 off-diagonal products once, double them and add the diagonal.  Plain C++ throughout; carries
// go through addc() below, written on __builtin_add_overflow (g++ and clang both have it) so that a chain becomes the machine's
// add-with-carry instead of 64-bit additions of zero-extended words: for 8 limbs that is 1 400 instructions a step instead of 2 000 and
// 118 registers instead of 196.
#ifndef FS_EXACT_MATH_HPP
#define FS_EXACT_MATH_HPP

#include <cstdint>

#if defined(__HIPCC__)
#define FSX_HD __host__ __device__ __forceinline__
#else
#define FSX_HD inline
#endif
#if defined(__clang__)
#define FSX_UNROLL _Pragma("unroll")
#else
#define FSX_UNROLL
#endif

// every instantiated limb count: frac_bits up to 32 * 24 - 10 = 758
#define FS_EXACT_FOR_EACH_L(X)                                                                                         \
    X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24)

namespace fsx {

constexpr uint32_t kMinLimbs = 2, kMaxLimbs = 24;
constexpr uint32_t kMaxBailout = 256; // integer R in 1 .. 256
constexpr uint32_t kCBoundLog2 = 5;   // |c| < 2^5

// the smallest limb count that holds frac_bits (not necessarily an instantiated one)
constexpr uint32_t limbs_for(uint32_t frac_bits) { return (frac_bits + 10 + 31) / 32; }

struct Params {
    uint32_t q, r;             // frac_bits = 32 q + r
    uint32_t bail_q;           // R * 2^(2 frac_bits) = (bail_hi : bail_lo) * 2^(32 bail_q)
    uint32_t bail_lo, bail_hi;
    uint32_t inclusive;        // escape at >= instead of >
};

inline Params make_params(uint32_t frac_bits, uint32_t R, int inclusive)
{
    Params P;
    P.q = frac_bits / 32, P.r = frac_bits % 32;
    P.bail_q = 2 * frac_bits / 32;
    const uint64_t b = (uint64_t)R << (2 * frac_bits % 32);
    P.bail_lo = (uint32_t)b, P.bail_hi = (uint32_t)(b >> 32);
    P.inclusive = inclusive ? 1u : 0u;
    return P;
}

// a + b + c with c = 0 or 1 going in; c = the carry coming out
FSX_HD uint32_t addc(uint32_t a, uint32_t b, uint32_t &c)
{
    uint32_t s, t;
    const uint32_t c1 = __builtin_add_overflow(a, b, &s) ? 1u : 0u;
    const uint32_t c2 = __builtin_add_overflow(s, c, &t) ? 1u : 0u;
    c = c1 | c2;
    return t;
}

// out = |x|; returns 1 when x is negative
template <int L> FSX_HD uint32_t magnitude(const uint32_t (&x)[L], uint32_t (&out)[L])
{
    const uint32_t neg = x[L - 1] >> 31, m = 0u - neg;
    uint32_t c = neg;
    FSX_UNROLL
    for (int i = 0; i < L; i++)
        out[i] = addc(x[i] ^ m, 0u, c);
    return neg;
}

// v = -v when neg (two's complement over N limbs)
template <int N> FSX_HD void negate_if(uint32_t (&v)[N], uint32_t neg)
{
    const uint32_t m = 0u - neg;
    uint32_t c = neg;
    FSX_UNROLL
    for (int i = 0; i < N; i++)
        v[i] = addc(v[i] ^ m, 0u, c);
}

// p = a * b, all 2L limbs
template <int L> FSX_HD void mul(const uint32_t (&a)[L], const uint32_t (&b)[L], uint32_t (&p)[2 * L])
{
    FSX_UNROLL
    for (int k = 0; k < 2 * L; k++)
        p[k] = 0;
    FSX_UNROLL
    for (int i = 0; i < L; i++) {
        uint64_t u[L];
        FSX_UNROLL
        for (int j = 0; j < L; j++)
            u[j] = (uint64_t)a[i] * b[j] + p[i + j]; // <= (2^32 - 1)^2 + 2^32 - 1
        p[i] = (uint32_t)u[0];
        uint32_t c = 0;
        FSX_UNROLL
        for (int j = 1; j < L; j++)
            p[i + j] = addc((uint32_t)u[j], (uint32_t)(u[j - 1] >> 32), c);
        p[i + L] = (uint32_t)(u[L - 1] >> 32) + c; // (column i + L is still empty; the total fits by the product's size)
    }
}

// p = a * a
template <int L> FSX_HD void square(const uint32_t (&a)[L], uint32_t (&p)[2 * L])
{
    FSX_UNROLL
    for (int k = 0; k < 2 * L; k++)
        p[k] = 0;
    // off-diagonal products a_i a_j, j > i, once
    FSX_UNROLL
    for (int i = 0; i + 1 < L; i++) {
        uint64_t u[L];
        FSX_UNROLL
        for (int j = i + 1; j < L; j++)
            u[j] = (uint64_t)a[i] * a[j] + p[i + j];
        p[2 * i + 1] = (uint32_t)u[i + 1];
        uint32_t c = 0;
        FSX_UNROLL
        for (int j = i + 2; j < L; j++)
            p[i + j] = addc((uint32_t)u[j], (uint32_t)(u[j - 1] >> 32), c);
        p[i + L] = (uint32_t)(u[L - 1] >> 32) + c;
    }
    // doubled (the sum of the off-diagonal products is below 2^(64L-1))
    FSX_UNROLL
    for (int k = 2 * L - 1; k > 0; k--)
        p[k] = (p[k] << 1) | (p[k - 1] >> 31);
    p[0] <<= 1;
    // plus the diagonal
    uint32_t c = 0;
    FSX_UNROLL
    for (int i = 0; i < L; i++) {
        const uint64_t d = (uint64_t)a[i] * a[i];
        p[2 * i] = addc(p[2 * i], (uint32_t)d, c);
        p[2 * i + 1] = addc(p[2 * i + 1], (uint32_t)(d >> 32), c);
    }
}

// whether the unsigned 2L-limb s exceeds (or, inclusive, reaches) R * 2^2F
template <int L> FSX_HD bool exceeds(const uint32_t (&s)[2 * L], const Params &P)
{
    bool gt = false, eq = true;
    FSX_UNROLL
    for (int i = 2 * L - 1; i >= 0; i--) {
        const uint32_t b = (uint32_t)i == P.bail_q ? P.bail_lo : ((uint32_t)i == P.bail_q + 1 ? P.bail_hi : 0u);
        gt = gt || (eq && s[i] > b);
        eq = eq && s[i] == b;
    }
    return gt || (P.inclusive && eq);
}

// out = floor(d / 2^F), d a two's-complement 2L-limb number whose quotient fits L limbs: an arithmetic shift right by 32 q + r
template <int L> FSX_HD void shift_floor(const uint32_t (&d)[2 * L], const Params &P, uint32_t (&out)[L])
{
    uint32_t t[L + 1];
    FSX_UNROLL
    for (int i = 0; i <= L; i++)
        t[i] = 0;
    // the limbs q .. q + L; q is the same for every lane, and every index is a constant
    FSX_UNROLL
    for (int qq = 0; qq < L; qq++)
        if (P.q == (uint32_t)qq) {
            FSX_UNROLL
            for (int i = 0; i <= L; i++)
                t[i] = d[i + qq];
        }
    FSX_UNROLL
    for (int i = 0; i < L; i++)
        out[i] = (uint32_t)((((uint64_t)t[i + 1] << 32) | t[i]) >> P.r);
}

// The escape test on z = (x, y) and, when it has not escaped, the step to its successor.  Returns true (z unchanged) on escape.
// norm(xx, yy, w) is handed the untruncated 2L-limb squares and their sum w = x^2 + y^2 of a z that has passed the test, before w's
// registers are used again (exact_atom_math.hpp keeps the smallest sum).
template <int L, class F>
FSX_HD bool step_with(uint32_t (&x)[L], uint32_t (&y)[L], const uint32_t (&cx)[L], const uint32_t (&cy)[L], const Params &P, F &&norm)
{
    uint32_t ax[L], ay[L];
    const uint32_t sx = magnitude<L>(x, ax), sy = magnitude<L>(y, ay);
    uint32_t xx[2 * L], yy[2 * L], w[2 * L];
    square<L>(ax, xx);
    square<L>(ay, yy);
    uint32_t c = 0;
    FSX_UNROLL
    for (int i = 0; i < 2 * L; i++)
        w[i] = addc(xx[i], yy[i], c);
    if (exceeds<L>(w, P))
        return true;
    norm(xx, yy, w);
    // x' = floor((x^2 - y^2) / 2^F) + cx
    c = 1; // xx + ~yy + 1
    FSX_UNROLL
    for (int i = 0; i < 2 * L; i++)
        w[i] = addc(xx[i], ~yy[i], c);
    shift_floor<L>(w, P, x);
    c = 0;
    FSX_UNROLL
    for (int i = 0; i < L; i++)
        x[i] = addc(x[i], cx[i], c);
    // y' = floor(2 x y / 2^F) + cy
    mul<L>(ax, ay, w);
    FSX_UNROLL
    for (int k = 2 * L - 1; k > 0; k--)
        w[k] = (w[k] << 1) | (w[k - 1] >> 31);
    w[0] <<= 1;
    negate_if<2 * L>(w, sx ^ sy);
    shift_floor<L>(w, P, y);
    c = 0;
    FSX_UNROLL
    for (int i = 0; i < L; i++)
        y[i] = addc(y[i], cy[i], c);
    return false;
}

template <int L>
FSX_HD bool step(uint32_t (&x)[L], uint32_t (&y)[L], const uint32_t (&cx)[L], const uint32_t (&cy)[L], const Params &P)
{
    return step_with<L>(x, y, cx, cy, P, [](const uint32_t (&)[2 * L], const uint32_t (&)[2 * L], const uint32_t (&)[2 * L]) {});
}

// The first n in 1 .. limit with |z_n|^2 > R (>= R), z_1 = c; 0 when there is none.  (Host loops and tests; the kernel keeps n itself.)
template <int L> FSX_HD uint64_t count(const uint32_t (&cx)[L], const uint32_t (&cy)[L], const Params &P, uint64_t limit)
{
    uint32_t x[L], y[L];
    FSX_UNROLL
    for (int i = 0; i < L; i++)
        x[i] = cx[i], y[i] = cy[i];
    for (uint64_t n = 1; n <= limit; n++)
        if (step<L>(x, y, cx, cy, P))
            return n;
    return 0;
}

} // namespace fsx

#endif
