// dw_math.hpp -- the double-word (head + tail) helpers of the direct low-precision kernels (kernels_direct_lp.hip): Gpu2x32's
// float-float and Gpu2x64's double-double arithmetic, and the declaration of the fused multiply-add rounded toward -infinity
// that Gpu1x32 calls.  Device code only.  Compiled with -ffp-contract=off: every operation below is one IEEE operation in
// source order, the fused ones are written as fma_rn.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

extern "C" __device__ __attribute__((const)) float __ocml_fma_rtn_f32(float, float, float);

namespace fs {

template <class T> struct dw {
    T h, t;
};
template <class T> __device__ __forceinline__ T fma_rn(T a, T b, T c);
template <> __device__ __forceinline__ float fma_rn<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <> __device__ __forceinline__ double fma_rn<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }

// add_float_to_dblflt / add_double_to_dbldbl (Knuth two-sum), dblflt.cuh:86-97, dbldbl.cuh:82-92
template <class T> __device__ __forceinline__ dw<T> two_sum(T a, T b)
{
    dw<T> z;
    z.h = a + b;
    T t1 = z.h - a;
    T t2 = z.h - t1;
    t1 = b - t1;
    t2 = a - t2;
    z.t = t1 + t2;
    return z;
}
// add_dblflt / add_dbldbl, dblflt.cuh:116-132, dbldbl.cuh:114-130
template <class T> __device__ __forceinline__ dw<T> dw_add(dw<T> a, dw<T> b)
{
    T t1 = a.h + b.h;
    T t2 = t1 - a.h;
    T t3 = (a.h + (t2 - t1)) + (b.h - t2);
    T t4 = a.t + b.t;
    t2 = t4 - a.t;
    const T t5 = (a.t + (t2 - t4)) + (b.t - t2);
    t3 = t3 + t4;
    t4 = t1 + t3;
    t3 = (t1 - t4) + t3;
    t3 = t3 + t5;
    const T e = t4 + t3;
    return dw<T>{e, (t4 - e) + t3};
}
// sub_dblflt / sub_dbldbl
template <class T> __device__ __forceinline__ dw<T> dw_sub(dw<T> a, dw<T> b)
{
    T t1 = a.h - b.h;
    T t2 = t1 - a.h;
    T t3 = (a.h + (t2 - t1)) - (b.h + t2);
    T t4 = a.t - b.t;
    t2 = t4 - a.t;
    const T t5 = (a.t + (t2 - t4)) - (b.t + t2);
    t3 = t3 + t4;
    t4 = t1 + t3;
    t3 = (t1 - t4) + t3;
    t3 = t3 + t5;
    const T e = t4 + t3;
    return dw<T>{e, (t4 - e) + t3};
}
// mul_dblflt / mul_dbldbl
template <class T> __device__ __forceinline__ dw<T> dw_mul(dw<T> a, dw<T> b)
{
    const T th = a.h * b.h;
    T tt = fma_rn<T>(a.h, b.h, -th);
    tt = fma_rn<T>(a.t, b.t, tt);
    tt = fma_rn<T>(a.h, b.t, tt);
    tt = fma_rn<T>(a.t, b.h, tt);
    const T e = th + tt;
    return dw<T>{e, (th - e) + tt};
}
// mul_dblflt2x, dblflt.cuh:178-192: the product with both parts doubled afterwards
__device__ __forceinline__ dw<float> dw_mul2x(dw<float> a, dw<float> b)
{
    dw<float> z = dw_mul(a, b);
    z.t = z.t * 2.0f;
    z.h = z.h * 2.0f;
    return z;
}
// sqr_dblflt, dblflt.cuh:194-214 (the cross term as one product doubled inside an fma)
__device__ __forceinline__ dw<float> dw_sqr(dw<float> a)
{
    const float th = a.h * a.h;
    float tt = fma_rn<float>(a.h, a.h, -th);
    tt = fma_rn<float>(a.t, a.t, tt);
    const float e0 = a.h * a.t;
    tt = fma_rn<float>(2.0f, e0, tt);
    const float e = th + tt;
    return dw<float>{e, (th - e) + tt};
}
// sqr_dbldbl, dbldbl.cuh:187-200 (the cross term as two fmas)
__device__ __forceinline__ dw<double> dw_sqr(dw<double> a)
{
    const double th = a.h * a.h;
    double tt = fma_rn<double>(a.h, a.h, -th);
    tt = fma_rn<double>(a.t, a.t, tt);
    tt = fma_rn<double>(a.h, a.t, tt);
    tt = fma_rn<double>(a.t, a.h, tt);
    const double e = th + tt;
    return dw<double>{e, (th - e) + tt};
}

} // namespace fs
#endif
