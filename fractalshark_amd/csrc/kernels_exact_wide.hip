// kernels_exact_wide.hip -- the wide exact renderer (fs_exact_sample_counts, fs_render_exact_wide, fs_exact_eval_points_wide,
// fs_exact_wide_state): the recurrence, the counting and the limb bound of exact_math.hpp with ONE WAVE PER SAMPLE, for limb counts no
// single lane can hold.
//
// A workgroup is one wave of 64 lanes and one sample.  With M = ceil(L / 64), every number of the recurrence is carried as
// 64 M limbs (two's complement, sign-extended above limb L - 1), lane t holding limbs t M .. t M + M - 1 ("block t"); a 128 M
// limb product is two such halves, lane t holding blocks t and t + 64.  The values are those of L-limb arithmetic: the bound of
// exact_math.hpp says every z fits L limbs and every product 2 L, and the padding above only repeats the sign.
//
//   product   schoolbook in M x M limb blocks.  In round s lane t multiplies block A_s -- read from lane s into scalar registers --
//             by block B_((t - s) mod 64), read from a copy of B in LDS.  The 2 M limb block product (fsx::mul<M>: rows of
//             independent 32 x 32 -> 64 multiply-adds and a carry chain each) is added into a lane-local accumulator of 2 M + 1
//             limbs.  Until round t that accumulator is column block t; in round t + 1 the rotation has wrapped for lane t: a copy
//             of the accumulator is kept, and what is added from then on is column block t + 64.  Blocks at and above ceil(L / M) of a
//             magnitude are zero, so the loop runs ceil(L / M) rounds, not 64.  Afterwards column block k lies over blocks k,
//             k + 1 and one limb of k + 2: the product is the sum of three numbers made of every lane's low M limbs, its
//             neighbour's next M limbs and the top limb from two lanes down.
//   addition  never ripples from lane to lane: block sums, two ballots, one 64-bit scalar addition (fsw::carry_in_mask), one
//             lane-local increment.  Subtraction, negation and magnitude are additions of the complement with carry-in 1.
//   shift     the 128 M limb value goes to LDS (512 M bytes); every lane reads back M + 1 limbs at the wave-uniform offset q and
//             funnel-shifts them by r.
//   escape    every lane compares its two blocks with the bailout value's; four ballots and the highest differing block decide.
//
// Slices as in kernels_exact.hip, with its lists (FsExactList of kernels.h, no checkpoints): a launch takes at most `slice` steps;
// a sample still running is written to the destination list (limb-major: plane l holds limb l of every slot) at a slot taken from
// one atomic add, so the next launch has exactly one wave per running sample.
//
// Keeping (K = true; fs_set_exact_keep): a sample that stops at n == cap + 1 is parked.  The kernel breaks BEFORE it steps, so the
// parked state is z_{cap+1} with n = cap + 1 -- a running sample's, and it resumes as one: the escape test on z_{cap+1} is made
// again (and counted again), nothing else.  All running samples hold the same n, so they meet the cap in one and the same slice,
// which has no survivor: the parked samples go to that slice's destination list, at slots counted by a counter of their own.
// K = false compiles to what it was without the parameter.
//
// Point runs (P = true, never with K; fs_exact_eval_points_wide): the point runs of kernels_exact.hip, one wave per run.  Run `id`
// stops at A.lengths[id] where a sample stops at A.cap.  The state that passes the escape test with n == lengths[id] goes to the
// end planes, limb g of x and y from the lane that holds it, before the step advances it.  The period rule (exact_atom_math.hpp)
// compares the norm the escape test has just formed with the run's smallest so far, all 128 blocks of both, as the escape test
// compares it with the bailout value: block by block in every lane, four ballots, the highest differing block decides
// (fsw::block_order, fsw::less_from_masks).  The minimum is held in 2 M registers while a slice runs; between slices it lives in
// the run's own limb planes (AtomPlanes::mn, indexed by id, not by slot: compaction copies nothing new), written by a run that is
// still running when its slice ends and read back when the next one starts.  No key: the full compare is one round of ballots.
// P = false compiles to what it was without the parameter.
#include <hip/hip_runtime.h>

#include "exact_atom_math.hpp"
#include "kernels.h"

namespace {

// s = a + b + cin over the 64 blocks; returns the carry out.  s may be a or b.
template <int M> __device__ __forceinline__ uint32_t wave_add(const uint32_t (&a)[M], const uint32_t (&b)[M], uint32_t cin, uint32_t lane,
                                                              uint32_t (&s)[M])
{
    const uint32_t g = fsw::block_add<M>(a, b, s);
    const uint64_t G = __ballot(g != 0), P = __ballot(fsw::block_all_ones<M>(s));
    uint32_t cout;
    const uint64_t C = fsw::carry_in_mask(G, P, cin, cout);
    fsw::block_inc<M>(s, (uint32_t)(C >> lane) & 1u);
    return cout;
}

// (slo, shi) = (alo, ahi) + (blo, bhi) + cin over 128 blocks, modulo 2^(32 * 128 M)
template <int M>
__device__ __forceinline__ void wave_add2(const uint32_t (&alo)[M], const uint32_t (&ahi)[M], const uint32_t (&blo)[M],
                                          const uint32_t (&bhi)[M], uint32_t cin, uint32_t lane, uint32_t (&slo)[M], uint32_t (&shi)[M])
{
    const uint32_t c = wave_add<M>(alo, blo, cin, lane, slo);
    (void)wave_add<M>(ahi, bhi, c, lane, shi);
}

// out = |x| over the 64 blocks; returns 1 when x is negative (the sign is bit 31 of lane 63's last limb)
template <int M> __device__ __forceinline__ uint32_t wave_magnitude(const uint32_t (&x)[M], uint32_t lane, uint32_t (&out)[M])
{
    const uint32_t neg = (uint32_t)__builtin_amdgcn_readlane((int)x[M - 1], 63) >> 31, m = 0u - neg;
    uint32_t t[M], z[M];
#pragma unroll
    for (int i = 0; i < M; i++)
        t[i] = x[i] ^ m, z[i] = 0;
    (void)wave_add<M>(t, z, neg, lane, out);
    return neg;
}

// (lo, hi) = a * b, a and b magnitudes whose blocks nb .. 63 are zero.  B goes to LDS once and every round reads the block it
// needs from there, so that no round waits for the one before it to hand B on and B holds no registers across the rounds (a B
// moved from lane to lane by ds_bpermute ran View 11's samples at the same pace, DESIGN.md 6.3: a lone wave's rounds are bound by
// their own dependent instructions, not by that round trip).
template <int M>
__device__ __forceinline__ void wave_mul(const uint32_t (&a)[M], const uint32_t (&b0)[M], uint32_t nb, uint32_t lane, uint32_t *lds,
                                         uint32_t (&lo)[M], uint32_t (&hi)[M])
{
    constexpr int N = 2 * M + 1;
    const int below = (int)((lane + 63u) & 63u), below2 = (int)((lane + 62u) & 63u);
    uint32_t cur[N], kept[N];
    __syncthreads(); // (whatever read the buffer before is done)
#pragma unroll
    for (int i = 0; i < M; i++)
        lds[lane * M + i] = b0[i];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++)
        cur[k] = 0, kept[k] = 0;
#pragma unroll 4
    for (uint32_t s = 0; s < nb; s++) {
        // From round t + 1 on lane t multiplies B_(t - s + 64): column block t + 64.  The sum goes on in the same registers (all 64
        // rounds together stay below 64 * 2^(64 M)); what it was when the rotation wrapped is kept, and taken off at the end.
        const bool wrapped_now = lane + 1u == s;
#pragma unroll
        for (int k = 0; k < N; k++)
            kept[k] = wrapped_now ? cur[k] : kept[k];
        uint32_t as[M], b[M], p[2 * M];
#pragma unroll
        for (int i = 0; i < M; i++) {
            as[i] = (uint32_t)__builtin_amdgcn_readlane((int)a[i], (int)s);
            b[i] = lds[((lane - s) & 63u) * M + i];
        }
        fsx::mul<M>(as, b, p);
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < 2 * M; k++)
            cur[k] = fsx::addc(cur[k], p[k], c);
        cur[2 * M] += c; // (at most 64 block products: the top limb stays below 64)
    }
    const bool wrapped = lane + 1u < nb;
    {
        // column block t = kept, column block t + 64 = cur - kept where the lane wrapped; cur and nothing where it did not
        uint32_t c = 1;
#pragma unroll
        for (int k = 0; k < N; k++) {
            const uint32_t d = fsx::addc(cur[k], ~kept[k], c);
            kept[k] = wrapped ? kept[k] : cur[k];
            cur[k] = wrapped ? d : 0u;
        }
    }
    uint32_t ylo[M], yhi[M], zlo[M], zhi[M];
#pragma unroll
    for (int i = 0; i < M; i++) {
        const uint32_t m0 = kept[M + i], m1 = cur[M + i];
        const uint32_t v0 = (uint32_t)__shfl((int)m0, below), v1 = (uint32_t)__shfl((int)m1, below);
        ylo[i] = lane == 0 ? 0u : v0;
        yhi[i] = lane == 0 ? v0 : v1; // (block 64 takes the middle of column block 63)
        lo[i] = kept[i];
        hi[i] = cur[i];
        zlo[i] = 0, zhi[i] = 0;
    }
    {
        const uint32_t t0 = kept[2 * M], t1 = cur[2 * M];
        const uint32_t v0 = (uint32_t)__shfl((int)t0, below2), v1 = (uint32_t)__shfl((int)t1, below2);
        zlo[0] = lane < 2 ? 0u : v0;
        zhi[0] = lane < 2 ? v0 : v1;
    }
    // (what lanes 62 and 63 hold above block 127 is zero: the product is below 2^(32 * 128 M))
    // (the top-limb number is zero above limb 0: a carry chain over constant zeros right behind an increment, the pattern
    // fsw::block_inc guards against)
    wave_add2<M>(lo, hi, ylo, yhi, 0, lane, lo, hi);
    wave_add2<M>(lo, hi, zlo, zhi, 0, lane, lo, hi);
}

// whether the unsigned 128-block s exceeds (or, inclusive, reaches) R * 2^2F
template <int M> __device__ __forceinline__ bool wave_exceeds(const uint32_t (&lo)[M], const uint32_t (&hi)[M], const fsx::Params &P, uint32_t lane)
{
    const uint32_t c0 = fsw::block_compare<M>(lo, lane * M, P), c1 = fsw::block_compare<M>(hi, (64u + lane) * M, P);
    return fsw::exceeds_from_masks(__ballot(c1 != 0), __ballot(c1 == 1), __ballot(c0 != 0), __ballot(c0 == 1), P.inclusive);
}

// out = floor(d / 2^(32 q + r)) over 64 blocks, d a two's-complement number of 128 blocks whose quotient fits: limbs q .. q + 64 M
// of d through LDS (q <= 64 M - 1, so the highest limb read is 128 M - 1)
template <int M>
__device__ __forceinline__ void wave_shift_floor(const uint32_t (&lo)[M], const uint32_t (&hi)[M], uint32_t q, uint32_t r, uint32_t lane,
                                                 uint32_t *lds, uint32_t (&out)[M])
{
    __syncthreads(); // (the reads of the shift before this one are done)
#pragma unroll
    for (int i = 0; i < M; i++) {
        lds[lane * M + i] = lo[i];
        lds[(64u + lane) * M + i] = hi[i];
    }
    __syncthreads();
    uint32_t t[M + 1];
#pragma unroll
    for (int i = 0; i <= M; i++)
        t[i] = lds[lane * M + q + i];
#pragma unroll
    for (int i = 0; i < M; i++)
        out[i] = (uint32_t)((((uint64_t)t[i + 1] << 32) | t[i]) >> r);
}

// limbs lane M .. lane M + M - 1 of value `idx` of a limb-major array, sign-extended above limb L - 1
template <int M>
__device__ __forceinline__ void load_blocks(const uint32_t *p, uint32_t stride, uint32_t idx, uint32_t L, uint32_t lane, uint32_t (&out)[M])
{
    const uint32_t ext = 0u - (p[(size_t)(L - 1) * stride + idx] >> 31);
#pragma unroll
    for (int i = 0; i < M; i++) {
        const uint32_t g = lane * M + i;
        out[i] = g < L ? p[(size_t)g * stride + idx] : ext;
    }
}

// whether the unsigned 128-block a is strictly below the unsigned 128-block b
template <int M>
__device__ __forceinline__ bool wave_below(const uint32_t (&alo)[M], const uint32_t (&ahi)[M], const uint32_t (&blo)[M], const uint32_t (&bhi)[M])
{
    const uint32_t c0 = fsw::block_order<M>(alo, blo), c1 = fsw::block_order<M>(ahi, bhi);
    return fsw::less_from_masks(__ballot(c1 != 0), __ballot(c1 == 2), __ballot(c0 != 0), __ballot(c0 == 2));
}

template <int M, bool K, bool P> __global__ void __launch_bounds__(64) k_exact_wide_slice(const FsExactWideArgs A)
{
    static_assert(!(K && P), "point runs are never kept");
    __shared__ uint32_t lds[128 * M];
    const uint32_t lane = threadIdx.x, slot = blockIdx.x, L = A.limbs;
    const uint32_t nb = (L + M - 1) / M;
    uint64_t n = 1;
    uint32_t id = slot;
    if (!A.first) {
        n = A.src.n[slot];
        id = A.src.id[slot];
    }
    const uint32_t ix = A.W ? id % A.W : id, iy = A.W ? id / A.W : id;
    uint32_t x[M], y[M], cx[M], cy[M];
    load_blocks<M>(A.cx, A.nx, ix, L, lane, cx);
    load_blocks<M>(A.cy, A.ny, iy, L, lane, cy);
    if (A.first) {
#pragma unroll
        for (int i = 0; i < M; i++)
            x[i] = cx[i], y[i] = cy[i];
    } else {
        load_blocks<M>(A.src.xy, A.stride, slot, L, lane, x);
        load_blocks<M>(A.src.xy + (size_t)L * A.stride, A.stride, slot, L, lane, y);
    }
    // point runs: the run's length in place of the cap, and its smallest norm so far (limbs 2L and up of a norm are zero; the first
    // slice has none yet, and the take at n = 1 asks for none)
    uint64_t cap = A.cap;
    uint32_t mnl[P ? M : 1], mnh[P ? M : 1];
    if constexpr (P) {
        cap = A.lengths[id];
#pragma unroll
        for (int i = 0; i < M; i++) {
            const uint32_t g = lane * M + i, gh = (64u + lane) * M + i;
            mnl[i] = !A.first && g < 2 * L ? A.periods->mn[(size_t)g * A.periods->stride + id] : 0u;
            mnh[i] = !A.first && gh < 2 * L ? A.periods->mn[(size_t)gh * A.periods->stride + id] : 0u;
        }
    }

    bool running = true, parked = false;
    uint32_t steps = 0;
    for (uint32_t k = 0; k < A.slice; k++) {
        // the escape test on z_n, on the untruncated sum
        uint32_t ax[M], ay[M], xxl[M], xxh[M], yyl[M], yyh[M], wl[M], wh[M];
        const uint32_t sx = wave_magnitude<M>(x, lane, ax), sy = wave_magnitude<M>(y, lane, ay);
        wave_mul<M>(ax, ax, nb, lane, lds, xxl, xxh);
        wave_mul<M>(ay, ay, nb, lane, lds, yyl, yyh);
        wave_add2<M>(xxl, xxh, yyl, yyh, 0, lane, wl, wh);
        const bool escaped = wave_exceeds<M>(wl, wh, A.P, lane);
        if (A.state_only) {
            if (escaped)
                break; // beyond the bound the limbs are sized for: this z is kept
        } else {
            steps++;
            if constexpr (P) {
                if (!escaped && n <= cap) { // (z_{cap+1} is tested, not tracked)
                    if (n == 1 || wave_below<M>(wl, wh, mnl, mnh)) {
#pragma unroll
                        for (int i = 0; i < M; i++)
                            mnl[i] = wl[i], mnh[i] = wh[i];
                        if (lane == 0)
                            A.periods->atom[id] = n;
                    }
                    if (n == cap) {
                        uint32_t *end = A.periods->end;
                        const uint32_t stride = A.periods->stride;
#pragma unroll
                        for (int i = 0; i < M; i++) {
                            const uint32_t g = lane * M + i;
                            if (g < L) {
                                end[(size_t)g * stride + id] = x[i];
                                end[(size_t)(L + g) * stride + id] = y[i];
                            }
                        }
                    }
                }
            }
            if (escaped || n == cap + 1) {
                if (lane == 0) {
                    const uint64_t v = escaped ? n - 1 : cap;
                    const size_t o = A.W ? (size_t)iy * A.out_pitch + ix : (size_t)id;
                    if (A.out_u64)
                        ((uint64_t *)A.out)[o] = v;
                    else
                        ((uint32_t *)A.out)[o] = (uint32_t)v;
                }
                running = false;
                if constexpr (K)
                    parked = !escaped;
                break;
            }
        }
        // x' = floor((x^2 - y^2) / 2^F) + cx
#pragma unroll
        for (int i = 0; i < M; i++)
            yyl[i] = ~yyl[i], yyh[i] = ~yyh[i];
        wave_add2<M>(xxl, xxh, yyl, yyh, 1, lane, wl, wh);
        wave_shift_floor<M>(wl, wh, A.P.q, A.P.r, lane, lds, x);
        (void)wave_add<M>(x, cx, 0, lane, x);
        // y' = floor(2 x y / 2^F) + cy
        wave_mul<M>(ax, ay, nb, lane, lds, wl, wh);
        wave_add2<M>(wl, wh, wl, wh, 0, lane, wl, wh);
        {
            const uint32_t neg = sx ^ sy, m = 0u - neg;
            uint32_t z[M];
#pragma unroll
            for (int i = 0; i < M; i++)
                wl[i] ^= m, wh[i] ^= m, z[i] = 0;
            wave_add2<M>(wl, wh, z, z, neg, lane, wl, wh);
        }
        wave_shift_floor<M>(wl, wh, A.P.q, A.P.r, lane, lds, y);
        (void)wave_add<M>(y, cy, 0, lane, y);
        n++;
    }

    if (running || (K && parked)) {
        uint32_t dst = slot;
        if (!A.state_only) {
            if (lane == 0)
                dst = atomicAdd(K && parked ? A.park_count : A.dst_count, 1u);
            dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)dst);
        }
#pragma unroll
        for (int i = 0; i < M; i++) {
            const uint32_t g = lane * M + i;
            if (g < L) {
                A.dst.xy[(size_t)g * A.stride + dst] = x[i];
                A.dst.xy[(size_t)(L + g) * A.stride + dst] = y[i];
            }
        }
        if (lane == 0) {
            A.dst.n[dst] = n;
            A.dst.id[dst] = id;
        }
        if constexpr (P) {
#pragma unroll
            for (int i = 0; i < M; i++) {
                const uint32_t g = lane * M + i, gh = (64u + lane) * M + i;
                if (g < 2 * L)
                    A.periods->mn[(size_t)g * A.periods->stride + id] = mnl[i];
                if (gh < 2 * L)
                    A.periods->mn[(size_t)gh * A.periods->stride + id] = mnh[i];
            }
        }
    }
    if (lane == 0 && steps != 0)
        atomicAdd(&A.stats[0], (unsigned long long)steps);
}

} // namespace

bool fsk_exact_wide_slice(const FsExactWideArgs &A, uint32_t n_src, bool keep, bool points, hipStream_t s)
{
    if (points && (keep || A.W != 0 || A.state_only || !A.periods || !A.lengths))
        return false;
    const dim3 grid(n_src), block(64);
    switch (fsw::block_for(A.limbs)) {
#define FS_EXACT_WIDE_CASE(M)                                                                                          \
    case M:                                                                                                             \
        if (points)                                                                                                     \
            hipLaunchKernelGGL((k_exact_wide_slice<M, false, true>), grid, block, 0, s, A);                             \
        else if (keep)                                                                                                  \
            hipLaunchKernelGGL((k_exact_wide_slice<M, true, false>), grid, block, 0, s, A);                             \
        else                                                                                                            \
            hipLaunchKernelGGL((k_exact_wide_slice<M, false, false>), grid, block, 0, s, A);                            \
        return true;
        FS_EXACT_WIDE_FOR_EACH_M(FS_EXACT_WIDE_CASE)
#undef FS_EXACT_WIDE_CASE
    default:
        return false;
    }
}
