// arith_ops.hpp -- one table of the arithmetic headers' functions, for the two small programs of tests/arith (arith_host.cpp, g++;
// arith_device.hip, hipcc gfx950) that evaluate a file of cases, one function call per case, and write the result's raw bits.
//
// A case is 17 words: the op id, then up to 16 operand words.  A result is 8 words.  float and int32 travel as one word, double as
// two (low word first), df32 as head, tail; hreal<F> as m, e; hcplx<F> as re, im, e; q4<T> as x, y, z, w; a pair as a, b.
//
// Each table entry is X(id, name, TA, TB, TC, expression in a, b, c): the operands are read in that order (`nil` reads nothing) and
// the expression's value is written.  tests/_arith_cases.py holds the same ids and the word counts; the CPU test compares the two
// tables through `arith_host --list`.
#pragma once

#include <stdint.h>

#include "../../fractalshark_amd/csrc/hdr_math.hpp"
#include "../../fractalshark_amd/csrc/df32_math.hpp"
#include "../../fractalshark_amd/csrc/qd_math.hpp"
#include "../../fractalshark_amd/csrc/bla_math.hpp"
#if defined(__HIPCC__)
#include "../../fractalshark_amd/csrc/dw_math.hpp"
#endif

namespace arith {

using fs::df32;
using fs::hcplx;
using fs::hreal;
using fs::q4;

static constexpr int kInWords = 16, kOutWords = 8, kCaseWords = 1 + kInWords;

struct nil {};
template <class T> struct pair2 {
    T a, b;
};

// ---------------------------------------------------------------- words in
FS_HD void ld(const uint32_t *&p, nil &) {}
FS_HD void ld(const uint32_t *&p, float &v) { v = fs::from_bits<float>(*p++); }
FS_HD void ld(const uint32_t *&p, int32_t &v) { v = (int32_t)*p++; }
FS_HD void ld(const uint32_t *&p, double &v)
{
    const uint64_t lo = p[0], hi = p[1];
    p += 2;
    v = fs::from_bits<double>(lo | (hi << 32));
}
FS_HD void ld(const uint32_t *&p, df32 &v)
{
    ld(p, v.head);
    ld(p, v.tail);
}
template <class F> FS_HD void ld(const uint32_t *&p, hreal<F> &v)
{
    ld(p, v.m);
    ld(p, v.e);
}
template <class F> FS_HD void ld(const uint32_t *&p, hcplx<F> &v)
{
    ld(p, v.re);
    ld(p, v.im);
    ld(p, v.e);
}
template <class T> FS_HD void ld(const uint32_t *&p, q4<T> &v)
{
    ld(p, v.x);
    ld(p, v.y);
    ld(p, v.z);
    ld(p, v.w);
}

// ---------------------------------------------------------------- words out
FS_HD void st(uint32_t *&o, float v) { *o++ = fs::to_bits<float>(v); }
FS_HD void st(uint32_t *&o, int32_t v) { *o++ = (uint32_t)v; }
FS_HD void st(uint32_t *&o, bool v) { *o++ = v ? 1u : 0u; }
FS_HD void st(uint32_t *&o, double v)
{
    const uint64_t u = fs::to_bits<double>(v);
    *o++ = (uint32_t)u;
    *o++ = (uint32_t)(u >> 32);
}
FS_HD void st(uint32_t *&o, df32 v)
{
    st(o, v.head);
    st(o, v.tail);
}
template <class F> FS_HD void st(uint32_t *&o, hreal<F> v)
{
    st(o, v.m);
    st(o, v.e);
}
template <class F> FS_HD void st(uint32_t *&o, hcplx<F> v)
{
    st(o, v.re);
    st(o, v.im);
    st(o, v.e);
}
template <class T> FS_HD void st(uint32_t *&o, q4<T> v)
{
    st(o, v.x);
    st(o, v.y);
    st(o, v.z);
    st(o, v.w);
}
template <class T> FS_HD void st(uint32_t *&o, pair2<T> v)
{
    st(o, v.a);
    st(o, v.b);
}

// ---------------------------------------------------------------- word counts (for --list)
template <class T> struct words;
template <> struct words<nil> { static constexpr int n = 0; };
template <> struct words<float> { static constexpr int n = 1; };
template <> struct words<int32_t> { static constexpr int n = 1; };
template <> struct words<bool> { static constexpr int n = 1; };
template <> struct words<double> { static constexpr int n = 2; };
template <> struct words<df32> { static constexpr int n = 2; };
template <class F> struct words<hreal<F>> { static constexpr int n = words<F>::n + 1; };
template <class F> struct words<hcplx<F>> { static constexpr int n = 2 * words<F>::n + 1; };
template <class T> struct words<q4<T>> { static constexpr int n = 4 * words<T>::n; };
template <class T> struct words<pair2<T>> { static constexpr int n = 2 * words<T>::n; };

// ---------------------------------------------------------------- by-reference functions as values
template <class T> FS_HD pair2<T> quick_two_sum(T a, T b)
{
    pair2<T> r;
    r.a = fs::q_quick_two_sum(a, b, r.b);
    return r;
}
template <class T> FS_HD pair2<T> two_sum_q(T a, T b)
{
    pair2<T> r;
    r.a = fs::q_two_sum(a, b, r.b);
    return r;
}
template <class T> FS_HD pair2<T> split(T a)
{
    pair2<T> r;
    fs::q_split(a, r.a, r.b);
    return r;
}
template <class T> FS_HD pair2<T> two_prod(T a, T b)
{
    pair2<T> r;
    r.a = fs::q_two_prod(a, b, r.b);
    return r;
}
template <class T> FS_HD pair2<T> two_sqr(T a)
{
    pair2<T> r;
    r.a = fs::q_two_sqr(a, r.b);
    return r;
}
template <class T> FS_HD q4<T> renorm(q4<T> c, T c4)
{
    fs::q_renorm(c.x, c.y, c.z, c.w, c4);
    return c;
}

#if defined(__HIPCC__)
template <class T> struct words<fs::dw<T>> { static constexpr int n = 2 * words<T>::n; };
template <class T> __device__ __forceinline__ void ld(const uint32_t *&p, fs::dw<T> &v)
{
    ld(p, v.h);
    ld(p, v.t);
}
template <class T> __device__ __forceinline__ void st(uint32_t *&o, fs::dw<T> v)
{
    st(o, v.h);
    st(o, v.t);
}
// two extended-exponent double-floats side by side, as hr_add2 takes them
struct hpair {
    hreal<df32> x, y;
};
struct add2_out {
    hreal<df32> x, y;
    bool rare;
};
template <> struct words<hpair> { static constexpr int n = 6; };
template <> struct words<add2_out> { static constexpr int n = 7; };
__device__ __forceinline__ void ld(const uint32_t *&p, hpair &v)
{
    ld(p, v.x);
    ld(p, v.y);
}
__device__ __forceinline__ void st(uint32_t *&o, add2_out v)
{
    st(o, v.x);
    st(o, v.y);
    st(o, v.rare);
}
template <bool kSubLo> __device__ __forceinline__ add2_out add2(hpair a, hpair b)
{
    bool rare = false;
    const fs::hreal2 r = fs::hr_add2<kSubLo>(fs::hreal2(a.x, a.y), fs::hreal2(b.x, b.y), rare);
    return add2_out{r.x(), r.y(), rare};
}
#endif

} // namespace arith

// ---------------------------------------------------------------- the table
// hdr_math.hpp, for every F; B is the id of the first entry
#define ARITH_HDR_COMMON(X, F, S, B)                                                                                      \
    X(B + 0, multiplier_##S, int32_t, nil, nil, fs::multiplier<F>(a))                                                     \
    X(B + 1, multiplier_neg_##S, int32_t, nil, nil, fs::multiplier_neg<F>(a))                                             \
    X(B + 2, hr_reduce_##S, hreal<F>, nil, nil, fs::hr_reduced(a))                                                        \
    X(B + 3, hr_from_mant_##S, F, nil, nil, fs::hr_from_mant<F>(a))                                                       \
    X(B + 5, hr_mul_##S, hreal<F>, hreal<F>, nil, fs::hr_mul(a, b))                                                       \
    X(B + 6, hr_mul2_##S, hreal<F>, nil, nil, fs::hr_mul2(a))                                                             \
    X(B + 8, hr_square_##S, hreal<F>, nil, nil, fs::hr_square(a))                                                         \
    X(B + 9, hr_add_##S, hreal<F>, hreal<F>, nil, fs::hr_add(a, b))                                                       \
    X(B + 10, hr_sub_##S, hreal<F>, hreal<F>, nil, fs::hr_sub(a, b))                                                      \
    X(B + 12, hr_abs_##S, hreal<F>, nil, nil, fs::hr_abs(a))                                                              \
    X(B + 13, hr_cmp_pos_##S, hreal<F>, hreal<F>, nil, (int32_t)fs::hr_cmp_pos(a, b))                                     \
    X(B + 14, hr_cmp_##S, hreal<F>, hreal<F>, nil, (int32_t)fs::hr_cmp(a, b))                                             \
    X(B + 15, hr_max_pos_##S, hreal<F>, hreal<F>, nil, fs::hr_max_pos(a, b))                                              \
    X(B + 16, hr_min_pos_##S, hreal<F>, hreal<F>, nil, fs::hr_min_pos(a, b))                                              \
    X(B + 17, hr_to_native_##S, hreal<F>, nil, nil, fs::hr_to_native(a))                                                  \
    X(B + 18, hc_from_hr_##S, hreal<F>, hreal<F>, nil, fs::hc_from_hr(a, b))                                              \
    X(B + 19, hc_from_native_##S, F, F, nil, fs::hc_from_native<F>(a, b))                                                 \
    X(B + 20, hc_add_##S, hcplx<F>, hcplx<F>, nil, fs::hc_add(a, b))                                                      \
    X(B + 21, hc_add_real_##S, hcplx<F>, hreal<F>, nil, fs::hc_add_real(a, b))                                            \
    X(B + 22, hc_mul_##S, hcplx<F>, hcplx<F>, nil, fs::hc_mul(a, b))                                                      \
    X(B + 23, hc_mul_real_##S, hcplx<F>, hreal<F>, nil, fs::hc_mul_real(a, b))                                            \
    X(B + 24, hc_mul2_##S, hcplx<F>, nil, nil, fs::hc_mul2(a))                                                            \
    X(B + 25, hc_reduce_##S, hcplx<F>, nil, nil, fs::hc_reduced(a))                                                       \
    X(B + 26, hc_norm2_##S, hcplx<F>, nil, nil, fs::hc_norm2(a))                                                          \
    X(B + 27, hc_cheb_##S, hcplx<F>, nil, nil, fs::hc_cheb(a))

// the entries that need `/`, sqrt or the bit layout of F: float and double only
#define ARITH_HDR_REAL(X, F, S, B)                                                                                        \
    X(B + 4, hr_from_number_##S, F, nil, nil, fs::hr_from_number<F>(a))                                                   \
    X(B + 7, hr_div_##S, hreal<F>, hreal<F>, nil, fs::hr_div(a, b))                                                       \
    X(B + 11, hr_recip_##S, hreal<F>, nil, nil, fs::hr_recip(a))                                                          \
    X(B + 28, hc_norm_##S, hcplx<F>, nil, nil, fs::hc_norm(a))                                                            \
    X(B + 29, hc_div_##S, hcplx<F>, hcplx<F>, nil, fs::hc_div(a, b))                                                      \
    X(B + 30, hc_recip_##S, hcplx<F>, nil, nil, fs::hc_recip(a))

#define ARITH_OPS_HDR(X)                                                                                                  \
    ARITH_HDR_COMMON(X, float, f32, 0)                                                                                    \
    ARITH_HDR_REAL(X, float, f32, 0)                                                                                      \
    ARITH_HDR_COMMON(X, double, f64, 40)                                                                                  \
    ARITH_HDR_REAL(X, double, f64, 40)                                                                                    \
    ARITH_HDR_COMMON(X, df32, df32, 80)

// df32_math.hpp (its multiplier / hr_reduce / hc_reduce specialisations are the df32 column above)
#define ARITH_OPS_DF32(X)                                                                                                 \
    X(120, df32_add, df32, df32, nil, a + b)                                                                              \
    X(121, df32_sub, df32, df32, nil, a - b)                                                                              \
    X(122, df32_neg, df32, nil, nil, -a)                                                                                  \
    X(123, df32_mul, df32, df32, nil, a * b)                                                                              \
    X(124, df32_lt, df32, df32, nil, a < b)                                                                               \
    X(125, df32_eq, df32, df32, nil, a == b)                                                                              \
    X(126, df32_gt, df32, df32, nil, a > b)                                                                               \
    X(127, df32_ge, df32, df32, nil, a >= b)                                                                              \
    X(128, df32_le, df32, df32, nil, a <= b)                                                                              \
    X(129, df32_fabs, df32, nil, nil, fs::fabs_bits<df32>(a))                                                             \
    X(130, hr2_from_float, float, nil, nil, fs::hr2_from_float(a))

// qd_math.hpp, for both scalar types
#define ARITH_QD(X, T, S, B)                                                                                              \
    X(B + 0, q_quick_two_sum_##S, T, T, nil, arith::quick_two_sum<T>(a, b))                                               \
    X(B + 1, q_two_sum_##S, T, T, nil, arith::two_sum_q<T>(a, b))                                                         \
    X(B + 2, q_split_##S, T, nil, nil, arith::split<T>(a))                                                                \
    X(B + 3, q_two_prod_##S, T, T, nil, arith::two_prod<T>(a, b))                                                         \
    X(B + 4, q_two_sqr_##S, T, nil, nil, arith::two_sqr<T>(a))                                                            \
    X(B + 5, q_renorm_##S, q4<T>, T, nil, arith::renorm<T>(a, b))                                                         \
    X(B + 6, q_add_##S, q4<T>, q4<T>, nil, a + b)                                                                         \
    X(B + 7, q_sub_##S, q4<T>, q4<T>, nil, a - b)                                                                         \
    X(B + 8, q_mul_scalar_##S, q4<T>, T, nil, a * b)                                                                      \
    X(B + 9, q_mul_##S, q4<T>, q4<T>, nil, a * b)                                                                         \
    X(B + 10, q_sqr_##S, q4<T>, nil, nil, fs::q_sqr(a))                                                                   \
    X(B + 11, q_mul_pwr2_##S, q4<T>, T, nil, fs::q_mul_pwr2(a, b))                                                        \
    X(B + 12, q_le_##S, q4<T>, q4<T>, nil, a <= b)                                                                        \
    X(B + 13, q_le_scalar_##S, q4<T>, T, nil, a <= b)

#define ARITH_OPS_QD(X)                                                                                                   \
    ARITH_QD(X, float, f32, 140)                                                                                          \
    ARITH_QD(X, double, f64, 170)

// bla_math.hpp's square-root users
#define ARITH_OPS_BLA(X)                                                                                                  \
    X(200, bla_sqrt_f32, hreal<float>, nil, nil, fs::bla_sqrt(a))                                                         \
    X(201, bla_hypot_f32, hreal<float>, hreal<float>, nil, fs::bla_hypot(a, b))                                           \
    X(202, bla_sqrt_f64, hreal<double>, nil, nil, fs::bla_sqrt(a))                                                        \
    X(203, bla_hypot_f64, hreal<double>, hreal<double>, nil, fs::bla_hypot(a, b))

// dw_math.hpp (device code only): the double-word helpers and the fused multiply-add toward -infinity as the kernel calls it
#define ARITH_DW(X, T, S, B)                                                                                              \
    X(B + 0, dw_two_sum_##S, T, T, nil, fs::two_sum<T>(a, b))                                                             \
    X(B + 1, dw_add_##S, fs::dw<T>, fs::dw<T>, nil, fs::dw_add(a, b))                                                     \
    X(B + 2, dw_sub_##S, fs::dw<T>, fs::dw<T>, nil, fs::dw_sub(a, b))                                                     \
    X(B + 3, dw_mul_##S, fs::dw<T>, fs::dw<T>, nil, fs::dw_mul(a, b))                                                     \
    X(B + 4, dw_sqr_##S, fs::dw<T>, nil, nil, fs::dw_sqr(a))

#define ARITH_OPS_DW(X)                                                                                                   \
    ARITH_DW(X, float, f32, 210)                                                                                          \
    X(215, dw_mul2x_f32, fs::dw<float>, fs::dw<float>, nil, fs::dw_mul2x(a, b))                                           \
    ARITH_DW(X, double, f64, 220)                                                                                         \
    X(230, fma_down_f32, float, float, float, __ocml_fma_rtn_f32(a, b, c))

// the packed pair of extended-exponent additions of the 2x32 perturbation step (device code only)
#define ARITH_OPS_ADD2(X)                                                                                                 \
    X(240, hr_add2_add, arith::hpair, arith::hpair, nil, arith::add2<false>(a, b))                                        \
    X(241, hr_add2_sub, arith::hpair, arith::hpair, nil, arith::add2<true>(a, b))

// [first id, last id] of each family: one launch per family in arith_device.hip
#define ARITH_FAMILIES(Y)                                                                                                 \
    Y(HDR, 0, 119)                                                                                                        \
    Y(DF32, 120, 139)                                                                                                     \
    Y(QD, 140, 199)                                                                                                       \
    Y(BLA, 200, 209)                                                                                                      \
    Y(DW, 210, 239)                                                                                                       \
    Y(ADD2, 240, 249)

// one case: read the operands in order, evaluate, write the value
#define ARITH_CASE(id, name, TA, TB, TC, expr)                                                                            \
    case id: {                                                                                                            \
        TA a;                                                                                                             \
        TB b;                                                                                                             \
        TC c;                                                                                                             \
        static_assert(arith::words<TA>::n + arith::words<TB>::n + arith::words<TC>::n <= arith::kInWords, #name);         \
        static_assert(arith::words<decltype(expr)>::n <= arith::kOutWords, #name);                                        \
        arith::ld(p, a);                                                                                                  \
        arith::ld(p, b);                                                                                                  \
        arith::ld(p, c);                                                                                                  \
        arith::st(o, (expr));                                                                                             \
        break;                                                                                                            \
    }
