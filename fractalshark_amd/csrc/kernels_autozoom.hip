// kernels_autozoom.hip -- the device side of fs_autozoom_pick: AutoZoomer::Run's scans of the iteration array
// (AutoZoomer.cpp:74-393) as streaming reductions next to the buffer the render kernels wrote.
//
// Shape of every kernel: ONE workgroup of 256 lanes per frame row (of the rectangle the heuristic looks at), lane t takes the
// pixels t, t + 256, ... of the row -- coalesced 4- or 8-byte loads, no division.  The grid is a function of the frame alone.
// Integer results (max, sum, counts, the first index, the largest score as an integer key) go through wave shuffles, one LDS
// hop and one integer atomic per workgroup (the pattern of k_reduce, kernels_current.hip): integer atomics give the same answer
// in whatever order they arrive.  The one heuristic with non-integer sums (Default) uses no atomic for them: a fixed tree per
// row into a slab, then one lane adds the slab in row order -- bitwise the same from run to run.
//
// The radius-12 samples of the FilamentTip classification are plain loads (L2): candidates are the pixels above the frame's
// average, and in frames where they are dense their samples are each other's rows, already in L2 from the row sweep.  An LDS
// tile with a 12-pixel halo (25 rows per row of output) was NOT tried.
#include <hip/hip_runtime.h>

#include "autozoom_math.hpp"
#include "kernels.h"

namespace {

constexpr uint32_t kBlock = 256;

__device__ inline uint64_t wave_sum(uint64_t v)
{
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off);
    return v;
}
__device__ inline uint64_t wave_max(uint64_t v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_down(v, off);
        v = o > v ? o : v;
    }
    return v;
}
__device__ inline uint64_t wave_min(uint64_t v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_down(v, off);
        v = o < v ? o : v;
    }
    return v;
}

// Pass 1: max, integer sum and count >= n_iterations over the rectangle.
template <class IterT>
__global__ void __launch_bounds__(kBlock) k_az_stats(const IterT *__restrict__ iters, uint32_t pitch, uint32_t x0, uint32_t y0,
                                                     uint32_t w, uint64_t n_iterations, FsAzStats *st)
{
    const IterT *row = iters + (size_t)(y0 + blockIdx.x) * pitch + x0;
    uint64_t mx = 0, sum = 0, ge = 0;
#pragma unroll 4
    for (uint32_t x = threadIdx.x; x < w; x += kBlock) {
        const uint64_t v = row[x];
        mx = v > mx ? v : mx;
        sum += v;
        ge += v >= n_iterations ? 1u : 0u;
    }
    mx = wave_max(mx), sum = wave_sum(sum), ge = wave_sum(ge);
    __shared__ uint64_t part[3][4];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0)
        part[0][wave] = mx, part[1][wave] = sum, part[2][wave] = ge;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < 4; k++) {
            mx = part[0][k] > mx ? part[0][k] : mx;
            sum += part[1][k];
            ge += part[2][k];
        }
        atomicMax((unsigned long long *)&st->max_iter, (unsigned long long)mx);
        atomicAdd((unsigned long long *)&st->sum, (unsigned long long)sum);
        if (ge)
            atomicAdd((unsigned long long *)&st->n_ge, (unsigned long long)ge);
    }
}

// Max, second pass: pixels at the maximum and the smallest linear index among them.
template <class IterT>
__global__ void __launch_bounds__(kBlock) k_az_max(const IterT *__restrict__ iters, uint32_t pitch, uint32_t W, FsAzStats *st)
{
    const uint64_t maxiter = st->max_iter;
    const IterT *row = iters + (size_t)blockIdx.x * pitch;
    uint64_t n = 0, first = ~0ull;
#pragma unroll 4
    for (uint32_t x = threadIdx.x; x < W; x += kBlock)
        if ((uint64_t)row[x] == maxiter) {
            n++;
            const uint64_t idx = (uint64_t)blockIdx.x * W + x;
            first = idx < first ? idx : first;
        }
    n = wave_sum(n), first = wave_min(first);
    __shared__ uint64_t part[2][4];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0)
        part[0][wave] = n, part[1][wave] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < 4; k++) {
            n += part[0][k];
            first = part[1][k] < first ? part[1][k] : first;
        }
        if (n) {
            atomicAdd((unsigned long long *)&st->num_at_limit, (unsigned long long)n);
            atomicMin((unsigned long long *)&st->first_index, (unsigned long long)first);
        }
    }
}

// Default, second pass (AutoZoomer.cpp:107-147) over one row of the rectangle.  The three sums: each lane adds its own pixels
// in x order, the lanes of a wave are folded by shuffles at distances 32, 16, ... 1, lane 0 adds the four waves in order and
// stores the row's triple to the slab.  No atomic touches a double.
template <class IterT>
__global__ void __launch_bounds__(kBlock) k_az_default(const IterT *__restrict__ iters, uint32_t pitch, uint32_t x0, uint32_t y0,
                                                       uint32_t w, uint32_t h, uint64_t n_iterations, double wo2, double ho2,
                                                       double max_distance, FsAzStats *st, double *__restrict__ slab)
{
    const uint64_t maxiter = st->max_iter;
    const double avg = (double)st->sum / (double)(int32_t)(h * w);
    const uint32_t yr = blockIdx.x; // row within the rectangle
    const IterT *row = iters + (size_t)(y0 + yr) * pitch + x0;
    const double dy = fabs(ho2 - fabs(ho2 - fabs((double)(int32_t)yr)));
    const double fy = (double)(int32_t)(y0 + yr);
    const double dN = (double)n_iterations;
    double s = 0, sx = 0, sy = 0;
    uint64_t at_limit = 0, at_max = 0;
    for (uint32_t xr = threadIdx.x; xr < w; xr += kBlock) {
        const IterT cur = row[xr];
        if ((uint64_t)cur == maxiter)
            at_limit++;
        if ((double)cur < avg)
            continue;
        const double dx = fabs(wo2 - fabs(wo2 - fabs((double)(int32_t)xr)));
        double ni = (double)cur / dN;
        if ((uint64_t)cur == maxiter)
            ni *= ni;
        const double nd = sqrt(dx * dx + dy * dy) / max_distance;
        const double sq = ni * nd;
        s += sq;
        sx += sq * (double)(int32_t)(x0 + xr);
        sy += sq * fy;
        if ((uint64_t)cur >= n_iterations)
            at_max++;
    }
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off);
        sx += __shfl_down(sx, off);
        sy += __shfl_down(sy, off);
    }
    at_limit = wave_sum(at_limit), at_max = wave_sum(at_max);
    __shared__ double dpart[3][4];
    __shared__ uint64_t ipart[2][4];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        dpart[0][wave] = s, dpart[1][wave] = sx, dpart[2][wave] = sy;
        ipart[0][wave] = at_limit, ipart[1][wave] = at_max;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < 4; k++) {
            s += dpart[0][k], sx += dpart[1][k], sy += dpart[2][k];
            at_limit += ipart[0][k], at_max += ipart[1][k];
        }
        slab[3u * yr] = s, slab[3u * yr + 1u] = sx, slab[3u * yr + 2u] = sy;
        if (at_limit)
            atomicAdd((unsigned long long *)&st->num_at_limit, (unsigned long long)at_limit);
        if (at_max)
            atomicAdd((unsigned long long *)&st->num_at_max, (unsigned long long)at_max);
    }
}

// Default, the small second step: the slab in row order, added by ONE lane.  The workgroup only fetches: 256 rows of the slab
// at a time into LDS with coalesced loads (a lone lane walking global memory waits out one load latency per row: measured
// 0.19 us per row, most of the heuristic's time), then lane 0 adds them in index order.
__global__ void __launch_bounds__(kBlock) k_az_default_finish(const double *__restrict__ slab, uint32_t rows, FsAzStats *st)
{
    __shared__ double tile[3u * kBlock];
    double s = 0, sx = 0, sy = 0;
    for (uint32_t base = 0; base < rows; base += kBlock) {
        const uint32_t n = rows - base < kBlock ? rows - base : kBlock;
        for (uint32_t i = threadIdx.x; i < 3u * n; i += kBlock)
            tile[i] = slab[3u * (size_t)base + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t k = 0; k < n; k++)
                s += tile[3u * k], sx += tile[3u * k + 1u], sy += tile[3u * k + 2u];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        st->sums[0] = s, st->sums[1] = sx, st->sums[2] = sy;
}

// FilamentTip (AutoZoomer.cpp:260-336): the 8 directions at radius 12 against cur - 1, the count of high ones and the longest
// run around the ring.  0 = more than 3 high, 1 = rejected for its run, 2 = accepted.  The margin (18) is wider than the
// radius, so no sample leaves the frame; the reference's test is kept, it costs nothing.
constexpr int kTipMargin = 18, kTipRadius = 12;
template <class IterT>
__device__ inline int tip_classify(const IterT *__restrict__ iters, uint32_t pitch, int W, int H, int x, int y, uint64_t cur,
                                   uint32_t *high_out)
{
    constexpr int ring_dx[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    constexpr int ring_dy[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
    const uint64_t thr = cur > 0 ? cur - 1 : cur;
    uint32_t mask = 0, high = 0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int sx = x + ring_dx[d] * kTipRadius, sy = y + ring_dy[d] * kTipRadius;
        if (sx < 0 || sx >= W || sy < 0 || sy >= H)
            continue;
        if ((uint64_t)iters[(size_t)sy * pitch + (uint32_t)sx] >= thr) {
            mask |= 1u << d;
            high++;
        }
    }
    *high_out = high;
    if (high > 3)
        return 0;
    int max_run = 0, run = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (mask >> (i & 7) & 1u) {
            run++;
            max_run = run > max_run ? run : max_run;
        } else {
            run = 0;
        }
    }
    if (high > 0 && max_run < (int)high)
        return 1;
    return 2;
}

// FilamentTip, scoring pass: one lane per pixel of the margin's interior classifies, counts and scores; the largest score of
// the launch goes out as an integer key (fs::az_key_of).  12 counters per lane: candidates, >= n_iterations, run rejects, the
// histogram; accepted = the candidates that are neither.
template <class IterT>
__global__ void __launch_bounds__(kBlock) k_az_tip_score(const IterT *__restrict__ iters, uint32_t pitch, uint32_t W, uint32_t H,
                                                         uint64_t n_iterations, double max_dist, FsAzStats *st)
{
    const double avg = (double)st->sum / (double)((uint64_t)W * H);
    const uint64_t threshold = (uint64_t)(avg + 1);
    const uint32_t y = kTipMargin + blockIdx.x;
    const IterT *row = iters + (size_t)y * pitch;
    uint32_t cnt[13] = {0}; // 0 candidates, 1 at max, 2 run rejects, 3 accepted, 4..12 histogram
    uint64_t best = 0;
    for (uint32_t x = kTipMargin + threadIdx.x; x < W - kTipMargin; x += kBlock) {
        const uint64_t cur = row[x];
        if (cur < threshold)
            continue;
        cnt[0]++;
        if (cur >= n_iterations)
            cnt[1]++;
        uint32_t high;
        const int c = tip_classify(iters, pitch, (int)W, (int)H, (int)x, (int)y, cur, &high);
#pragma unroll
        for (uint32_t k = 0; k < 9; k++)
            cnt[4 + k] += high == k ? 1u : 0u;
        if (c == 1)
            cnt[2]++;
        if (c != 2)
            continue;
        cnt[3]++;
        const uint64_t key = fs::az_key_of(fs::az_tip_score(cur, high, x, y, W, H, n_iterations, avg, max_dist));
        best = key > best ? key : best;
    }
    __shared__ uint32_t total[13];
    __shared__ unsigned long long best_s;
    if (threadIdx.x < 13)
        total[threadIdx.x] = 0;
    if (threadIdx.x == 0)
        best_s = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 13; k++) {
        uint32_t v = cnt[k];
        for (int off = 32; off > 0; off >>= 1)
            v += __shfl_down(v, off);
        if ((threadIdx.x & 63u) == 0 && v)
            atomicAdd(&total[k], v);
    }
    best = wave_max(best);
    if ((threadIdx.x & 63u) == 0 && best)
        atomicMax(&best_s, (unsigned long long)best);
    __syncthreads();
    if (threadIdx.x < 13 && total[threadIdx.x]) {
        uint64_t *dst = threadIdx.x == 0 ? &st->candidates
                        : threadIdx.x == 1 ? &st->num_at_max
                        : threadIdx.x == 2 ? &st->run_reject
                        : threadIdx.x == 3 ? &st->accepted
                                           : &st->hist[threadIdx.x - 4];
        atomicAdd((unsigned long long *)dst, (unsigned long long)total[threadIdx.x]);
    }
    if (threadIdx.x == 0 && best_s)
        atomicMax((unsigned long long *)&st->best_key, best_s);
}

// How far below the device maximum a candidate's device score may lie and still be the host's winner.  Host and device scores
// are the same IEEE operations on the same inputs except for the two log() calls, each good to a few ulp on either side
// (OCML documents 1 ulp for f64 log; glibc's is below 1 ulp), so raw = log / log differs by at most ~8 ulp(raw) between the
// sides, and the score -- raw times factors of magnitude <= 1 -- by e <= 8 * 2^-52 * max(1, raw).  A candidate can only win on
// the host with a host score above -1, i.e. raw < 1 + 1 / (0.25 * 0.3) < 15, so e < 2^-45.  The host's winner w has
// device(w) >= host(w) - e >= host(m) - e >= device(m) - 2 e for the device's best m: within 2^-44 of the device maximum, and
// so is every candidate that ties with it on the host.  2^-40 leaves a factor of 16 on top.  The margin is ABSOLUTE: the
// score is tipness * (1 - raw) * ..., and 1 - raw cancels, so an error relative to raw is not relative to the score.
constexpr double kTipGatherMargin = 0x1p-40;

template <class IterT>
__global__ void __launch_bounds__(kBlock) k_az_tip_gather(const IterT *__restrict__ iters, uint32_t pitch, uint32_t W, uint32_t H,
                                                          uint64_t n_iterations, double max_dist, uint32_t ya, FsAzStats *st,
                                                          FsAzTipRec *__restrict__ out, uint32_t cap,
                                                          uint32_t *__restrict__ row_counts)
{
    const uint64_t best_key = st->best_key;
    if (!best_key)
        return; // no accepted candidate
    const double floor_score = fs::az_double_of(best_key) - kTipGatherMargin;
    const double avg = (double)st->sum / (double)((uint64_t)W * H);
    const uint64_t threshold = (uint64_t)(avg + 1);
    const uint32_t y = ya + blockIdx.x;
    const IterT *row = iters + (size_t)y * pitch;
    for (uint32_t x = kTipMargin + threadIdx.x; x < W - kTipMargin; x += kBlock) {
        const uint64_t cur = row[x];
        if (cur < threshold)
            continue;
        uint32_t high;
        if (tip_classify(iters, pitch, (int)W, (int)H, (int)x, (int)y, cur, &high) != 2)
            continue;
        if (!(fs::az_tip_score(cur, high, x, y, W, H, n_iterations, avg, max_dist) >= floor_score))
            continue;
        const unsigned long long slot = atomicAdd((unsigned long long *)&st->gathered, 1ull);
        if (slot < cap)
            out[slot] = FsAzTipRec{x, y, cur, high, 0u};
        if (row_counts)
            atomicAdd(&row_counts[y], 1u);
    }
}

} // namespace

#define FS_AZ_LAUNCH(kernel, grid, ...)                                                                                            \
    do {                                                                                                                           \
        if (F.iter_u64)                                                                                                            \
            hipLaunchKernelGGL(kernel<uint64_t>, dim3(grid), dim3(kBlock), 0, s, (const uint64_t *)F.iters, __VA_ARGS__);          \
        else                                                                                                                       \
            hipLaunchKernelGGL(kernel<uint32_t>, dim3(grid), dim3(kBlock), 0, s, (const uint32_t *)F.iters, __VA_ARGS__);          \
    } while (0)

void fsk_az_stats(const FsAzFrame &F, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, FsAzStats *st, hipStream_t s)
{
    if (!w || !h || x0 + w > F.W || y0 + h > F.H)
        return;
    FS_AZ_LAUNCH(k_az_stats, h, F.pitch, x0, y0, w, F.n_iterations, st);
}

void fsk_az_max(const FsAzFrame &F, FsAzStats *st, hipStream_t s)
{
    if (!F.W || !F.H)
        return;
    FS_AZ_LAUNCH(k_az_max, F.H, F.pitch, F.W, st);
}

void fsk_az_default(const FsAzFrame &F, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, double width_over_2,
                    double height_over_2, double max_distance, FsAzStats *st, double *slab, hipStream_t s)
{
    if (!w || !h || x0 + w > F.W || y0 + h > F.H)
        return;
    FS_AZ_LAUNCH(k_az_default, h, F.pitch, x0, y0, w, h, F.n_iterations, width_over_2, height_over_2, max_distance, st, slab);
    hipLaunchKernelGGL(k_az_default_finish, dim3(1), dim3(kBlock), 0, s, (const double *)slab, h, st);
}

void fsk_az_tip_score(const FsAzFrame &F, double max_dist, FsAzStats *st, hipStream_t s)
{
    if (F.W <= 2u * kTipMargin || F.H <= 2u * kTipMargin)
        return;
    FS_AZ_LAUNCH(k_az_tip_score, F.H - 2u * kTipMargin, F.pitch, F.W, F.H, F.n_iterations, max_dist, st);
}

void fsk_az_tip_gather(const FsAzFrame &F, double max_dist, uint32_t ya, uint32_t yb, FsAzStats *st, FsAzTipRec *out,
                       uint32_t cap, uint32_t *row_counts, hipStream_t s)
{
    if (F.W <= 2u * kTipMargin || F.H <= 2u * kTipMargin || ya < (uint32_t)kTipMargin || yb > F.H - kTipMargin || ya >= yb)
        return;
    FS_AZ_LAUNCH(k_az_tip_gather, yb - ya, F.pitch, F.W, F.H, F.n_iterations, max_dist, ya, st, out, cap, row_counts);
}
