// kernels_orbit_prep.hip -- what an uploaded HDRFloat<float | double> reference orbit becomes before a kernel reads it: the
// prepared entries (the complex form the CPU loop rebuilds on every access, made once per upload), and for HDRFloat<float> the
// companion arrays of the tuned loops' quiet and scaled runs, with the proofs of the bounds they carry.
// Compiled with -ffp-contract=off (see hdr_math.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fs_layout.h"
#include "hdr_math.hpp"
#include "kernels.h"
#include "lav2_common.hpp"
#include "scaled_runs.hpp"

using namespace fs;

// ------------------------------------------------------------------------------------------------
// Orbit preparation: fs_orbit_hdr32 (reference layout) -> {re, im, exp, 2^(8 - 2 exp)} (zref_pack, lav2_common.hpp).
__global__ void k_prepare_orbit_hdr32(const fs_orbit_hdr32 *__restrict__ in, float4 *__restrict__ out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const fs_orbit_hdr32 e = in[i];
    out[i] = zref_pack(hc_from_hr(hreal32{e.mx, e.ex}, hreal32{e.my, e.ey}));
}

// Orbit preparation for HDRFloat<double>.
__global__ void k_prepare_orbit_hdr64(const fs_orbit_hdr64 *__restrict__ in, FsZ64 *__restrict__ out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const fs_orbit_hdr64 e = in[i];
    out[i] = zref_pack(hc_from_hr(hreal64{e.mx, e.ex}, hreal64{e.my, e.ey}));
}

// Bound of a scaled-run arrival at orbit entry v = {re, im, exp}: 2^-2 * max(|Z.re|, |Z.im|) in true scale, or -0.0 (bit
// pattern INT_MIN = "never": the loops compare bit patterns as integers) unless 2^-40 <= max part < 5.6 (|Z| < 8) and the
// smaller part is within 2^40 of the larger one.
__device__ __forceinline__ float scaled_bound(const float4 v)
{
    const int e = __float_as_int(v.z);
    const float hi = fs_max_abs(v.x, v.y);
    const float lo = fs_min_abs(v.x, v.y);
    const float zmax = __builtin_amdgcn_ldexpf(hi, e < -200 ? -200 : (e > 100 ? 100 : e));
    const bool usable = zmax >= 0x1p-40f && zmax < 5.6f && lo >= hi * 0x1p-40f;
    return usable ? zmax * 0x1p-2f : -0.0f;
}


// Companion array of the tuned LAv2 loop: {re, im, s, -} with s = ~exp + 116 (-(s - 116) = exp + 1 = the exponent of 2Z;
// the bias turns the loop's range tests into comparisons against constants) for orbit values below 8, and a large
// positive poison for larger ones, which makes the range test fail there.  zq must hold 2 n entries.
// Block bound of entry j (the .w of the second companion, see below; "never" when one of the four entries after j has no
// bound).  With G = max(max|dz|, max|dc|) at entry j (maximum norms of the parts, true scale) the block's four arrivals pass
// their own bound tests whenever G <= this value:
//   one step from entry k:  dz' = dz (2 Z_k + dz) + dc,  |a b|_inf <= 2 |a|_inf |b|_inf for complex a, b, so
//   |dz'|_inf <= 2 G (2 M_k + G) + G <= G (4 M_k + 3.8)        M_k = max part of Z_k,  G <= 1.4 (every bound is <= 0.25 * 5.6)
//   => G grows by at most g_k = 4 M_k + 3.8 per step (dc included: g_k > 1), and arrival j + m passes its test when
//      G g_j g_(j+1) .. g_(j+m-1) <= bound[j + m]:   block bound = min over m = 1 .. 4 of bound[j + m] / (g_j .. g_(j+m-1)),
//   by induction over the block's steps (arrival j + m - 1 has passed its test, so G <= 1.4 holds where step m starts; at
//   entry j itself G <= bound[j + 1] / 3.8).  Rounding: the steps' own rounding errors are 2^-23 relative, each g carries
//   a factor 1 + 2^-10.  (Round 3 used one constant for every step -- |2Z + dz| < 20, i.e. 2^-18 for four steps; the orbit's
//   own |Z| gives 2^-9 .. 2^-12 for typical entries, and fewer blocks need their bound tests.)
__device__ __forceinline__ float scaled_block_bound(const float4 *__restrict__ zref, uint64_t j, uint64_t n)
{
    if (j >= n)
        return -0.0f;
    float best = 0x1p60f, grow = 1.0f;
    bool ok = true;
    for (uint32_t k = 0; k < 4; k++) {
        // growth of the step that leaves entry j + k
        const float4 v = zref[j + k < n ? j + k : n - 1];
        const int e = __float_as_int(v.z);
        const float m = __builtin_amdgcn_ldexpf(fs_max_abs(v.x, v.y),
                                               e < -200 ? -200 : (e > 100 ? 100 : e));
        ok = ok && m < 5.6f; // (a state never sits at an entry this large: its own bound is "never")
        grow *= (4.0f * m + 3.8f) * (1.0f + 0x1p-10f);
        const float bk = j + k + 1 < n ? scaled_bound(zref[j + k + 1]) : -0.0f;
        ok = ok && __float_as_int(bk) != (int)0x80000000;
        best = __builtin_fminf(best, bk / grow);
    }
    return ok ? best * (1.0f - 0x1p-10f) : -0.0f;
}

// NDZ body bounds of entry j (third companion of the scaled runs, `znz`; FS_FAST_LOOP_FDU's bodies without the dz add, whose
// comment in scaled_runs.hpp carries the argument): with D = max|dz| <= .x and C = max|dc| <= .y at entry j, each of the eight steps
// that leave the entries j .. j + 7 computes fma(w, 2^E, 2Z) == 2Z in both parts, and all eight arrivals pass their bound tests.
// dc has a term of its own.  With lo = min(|2Z.re|, |2Z.im|), 2Z as the loop reads it (the second companion's .xy), and the growth an
// NDZ step really has, s_k = (|2Z_k.re| + |2Z_k.im|)(1 + 2^-10):
//   A_0 = 1, B_0 = 0,  A_(m+1) = s_(j+m) A_m,  B_(m+1) = s_(j+m) B_m + 1      (A_m = the product of the s, B_m = the sum over i of the
//                                                                              products of the s after step i)
//   .x = min over m = 0 .. 7 of 2^-27 lo_(j+m) / A_m,   .y = min over m = 1 .. 7 of 2^-27 lo_(j+m) / B_m,
//   each also within half of scaled_bound(Z_(j+8)) over A_8 / B_8 (the eighth arrival's own bound test), times (1 - 2^-10).
// Induction over the body's steps, hypothesis at m:  max|dz_m| <= A_m D + B_m C <= 2^-26 lo_(j+m)  (both halves <= 2^-27 lo).
//   => s = fl(2Z + dz_m) == 2Z in both parts (|dz part| <= 2^-26 |2Z part|; fl(a + d) == a for |d| <= 2^-26 |a|), so
//      dz_(m+1) = dz_m 2Z + dc as written, |re| = |dz.re 2Z.re - dz.im 2Z.im + dc.re| <= (|2Z.re| + |2Z.im|) |dz_m|_inf + |dc|_inf, the
//      imaginary part alike; the two products and the two sums round 2^-24 relative each, which 1 + 2^-10 covers:
//      max|dz_(m+1)| <= s (A_m D + B_m C) + C = A_(m+1) D + B_(m+1) C
//   => the hypothesis at m + 1 by the terms m + 1 of .x and .y, for m + 1 <= 7
//   => arrival m + 1 passes its bound test: max|dz_(m+1)| <= 2^-26 lo <= 2^-25 zmax <= 2^-2 zmax, its scaled_bound, because entry
//      j + m + 1 is usable (lo <= 2 zmax); the eighth arrival by the halves of scaled_bound(Z_(j+8)).
// (Round 8 kept ONE bound on max(max|dz|, max|dc|) and divided by scaled_block_bound's g_k = 4 M_k + 3.8, valid for any G <= 1.4:
// 2^18 .. 2^21 over seven typical steps.  One bound with the growth s + 1 -- dc riding on dz's term -- gave 2^9 .. 2^13 and took NDZ
// from 52.0 % to 71.4 % of the statement's wave-steps on the C3 frame; its counting launch found 1.65e8 more wave-steps for the two
// terms, 0.95 % of the launch's vector instructions at 1.25 each, above the 0.8 % that was set for building them.)
// Neither bound is within scaled_block_bound(j) or (j + 4) by construction, and needs not be: an NDZ body has no test inside and the
// induction vouches for its arrivals.  "Never" (both): one of the entries j + 1 .. j + 8 without a usable bound or an M >= 5.6 among
// j .. j + 7 (either block bound says so; this covers j + 8 >= n), a part of a 2Z zero or not safely normal (< 2^-100), or a result
// below 2^-120 or not finite: the loops compare bit patterns as integers, which orders normal numbers only.
__device__ __forceinline__ float2 ndz_body_bound(const float4 *__restrict__ zref, uint64_t j, uint64_t n)
{
    const float2 never = make_float2(-0.0f, -0.0f);
    if (j + 8 >= n)
        return never;
    const float b0 = scaled_block_bound(zref, j, n), b4 = scaled_block_bound(zref, j + 4, n);
    if (__float_as_int(b0) == (int)0x80000000 || __float_as_int(b4) == (int)0x80000000)
        return never;
    float bd = 0x1p60f, bc = 0x1p60f, a = 1.0f, b = 0.0f;
    bool ok = true;
    for (uint32_t m = 0; m < 8; m++) {
        const float4 v = zref[j + m];
        const int e = __float_as_int(v.z);
        // 2Z as the loop reads it (the second companion's .xy)
        const float zr = __builtin_fabsf(__builtin_amdgcn_ldexpf(v.x, e + 1)), zi = __builtin_fabsf(__builtin_amdgcn_ldexpf(v.y, e + 1));
        const float lo = __builtin_fminf(zr, zi);
        ok = ok && lo >= 0x1p-100f;
        bd = __builtin_fminf(bd, lo * 0x1p-27f / a);
        if (m != 0)
            bc = __builtin_fminf(bc, lo * 0x1p-27f / b);
        // growth of the step that leaves entry j + m (every part here is below 11.2: the block bounds are not "never")
        const float s = (zr + zi) * (1.0f + 0x1p-10f);
        b = s * b + 1.0f;
        a *= s;
    }
    const float sb = scaled_bound(zref[j + 8]) * 0.5f;
    bd = __builtin_fminf(bd, sb / a) * (1.0f - 0x1p-10f);
    bc = __builtin_fminf(bc, sb / b) * (1.0f - 0x1p-10f);
    ok = ok && bd >= 0x1p-120f && bd < 0x1p60f && bc >= 0x1p-120f && bc < 0x1p60f;
    return ok ? make_float2(bd, bc) : never;
}

__global__ void k_make_quiet_orbit(const float4 *__restrict__ zref, float4 *__restrict__ zq, float2 *__restrict__ zs2,
                                   float4 *__restrict__ zqb, float2 *__restrict__ znz, uint64_t n, uint64_t slack)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // (the slack behind the NDZ bounds is requested a body ahead and never used; it reads as "never" all the same)
    if (i < slack)
        znz[n + i] = make_float2(-0.0f, -0.0f);
    if (i >= n)
        return;
    const float4 v = zref[i];
    const int e = __float_as_int(v.z);
    zq[i] = make_float4(v.x, v.y, __int_as_float(e <= 2 ? ~e + 116 : (1 << 24)), 0.0f);
    // second companion, zq[n + i], for the scaled runs: {2Z.re, 2Z.im, scaled_bound(Z), block bound} as plain floats (true
    // scale).  (Packing the entry into 8 bytes and deriving the bound from 2Z costs one more vector
    // instruction per step and was measured slower: the loop is not bound by its loads.)
    const float b0 = scaled_bound(v);
    // .w: the BLOCK bound of the four entries after this one (scaled_block_bound above): G = max(max|dz|, max|dc|) <= .w at
    // this entry implies that each of the four arrivals passes its own bound test, and the scalar-cache path of the scaled
    // runs then skips those tests (same accepted steps).  (Eight entries per test -- one test per loop body -- passed for
    // 67 % of C3's blocks instead of 93.6 % with round 3's constant-growth bound: 63.5 instead of 55.8 ms.)
    // (A run may START at every usable entry and at an exact zero -- entry 0, where every rebase lands; 2Z + dz is then dz
    // itself in either arithmetic -- the kernels read that off .z and .xy.  Nothing arrives at a zero entry: its bound is
    // the "never" pattern.)
    zq[n + i] = make_float4(__builtin_amdgcn_ldexpf(v.x, e + 1), __builtin_amdgcn_ldexpf(v.y, e + 1), b0,
                            scaled_block_bound(zref, i, n));
    // the compact form for the 16-step body of the untested loop (FS_FAST_LOOP_FD16P): 2Z alone, and the block bounds a body
    // whose first arrival is entry i needs -- those of its entries 3, 7, 11 (the states its second to fourth blocks start
    // from) and 15 (the state the NEXT body starts from)
    zs2[i] = make_float2(__builtin_amdgcn_ldexpf(v.x, e + 1), __builtin_amdgcn_ldexpf(v.y, e + 1));
    zqb[i] = make_float4(scaled_block_bound(zref, i + 3, n), scaled_block_bound(zref, i + 7, n),
                         scaled_block_bound(zref, i + 11, n), scaled_block_bound(zref, i + 15, n));
    znz[i] = ndz_body_bound(zref, i, n);
}

// ------------------------------------------------------------------------------------------------
// Host-callable launchers (called from renderer_inputs.cpp through kernels.h).
void fsk_prepare_orbit_hdr32(const fs_orbit_hdr32 *in, float4 *out, uint64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_prepare_orbit_hdr32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
}

void fsk_make_quiet_orbit(const float4 *zref, float4 *zq, float2 *zs2, float4 *zqb, float2 *znz, uint64_t n, hipStream_t s)
{
    // (n >= 32 or not: the first block alone has more threads than the 32 entries of slack)
    hipLaunchKernelGGL(k_make_quiet_orbit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, zref, zq, zs2, zqb, znz, n,
                       (uint64_t)32);
}

void fsk_prepare_orbit_hdr64(const fs_orbit_hdr64 *in, FsZ64 *out, uint64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_prepare_orbit_hdr64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
}
