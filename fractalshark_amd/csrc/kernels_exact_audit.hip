// kernels_exact_audit.hip -- fs_exact_audit's second kernel: the frame at the sample pixels against the counts their runs left
// (exact_audit_math.hpp holds the rule).  ONE workgroup of one wave walks the samples in index order, 64 at a time: every lane
// classifies its sample, ballots turn the lanes' answers into masks, and lane 0 adds the chunk to the record in LDS -- popcounts
// for the sums, a prefix count for an offender's place, a butterfly maximum for max_abs_diff.  No atomics: the record is the same
// from run to run.  n_samples is thousands, so the walk's time is nothing next to the runs'; what matters is that the frame is read
// where it lies and only the record leaves the device.
#include <hip/hip_runtime.h>

#include "exact_audit_math.hpp"
#include "kernels.h"

namespace {

__global__ void __launch_bounds__(64) k_exact_audit(const FsAuditArgs A)
{
    __shared__ fs_audit_result R;
    const uint32_t lane = threadIdx.x;
    for (uint32_t w = lane; w < sizeof(fs_audit_result) / 4; w += 64u)
        ((uint32_t *)&R)[w] = 0;
    __syncthreads();
    if (lane == 0)
        R.n_samples = A.n_samples, R.n_levels = A.n_levels;
    __syncthreads();

    for (uint32_t base = 0; base < A.n_samples; base += 64u) {
        const uint32_t i = base + lane;
        const bool valid = i < A.n_samples;
        fsa::Sample s{};
        if (valid) {
            s = fsa::classify(A.counts, A.n_samples, A.n_levels, i, fsa::frame_at(A.iters, A.iter_u64, A.pitch, A.xs[i], A.ys[i]),
                              A.cap);
            A.exact[i] = s.exact;
            A.frame[i] = s.frame;
            A.stable[i] = s.stable_bits;
        }
        const uint64_t m_valid = __ballot(valid), m_differ = __ballot(valid && s.differ), m_capped = __ballot(valid && s.capped);
        uint64_t m_stable[FS_AUDIT_MAX_LEVELS], level_max[FS_AUDIT_MAX_LEVELS];
#pragma unroll
        for (uint32_t j = 0; j < FS_AUDIT_MAX_LEVELS; j++) {
            m_stable[j] = __ballot(valid && ((s.stable_bits >> j) & 1u));
            uint64_t d = valid ? fsa::level_diff(s, j) : 0ull;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint64_t o = __shfl_xor(d, off);
                d = o > d ? o : d;
            }
            level_max[j] = d;
        }
        const uint32_t before = R.n_differ; // (read by every lane before lane 0 adds the chunk)
        __syncthreads();
        if (valid && s.differ) {
            const uint32_t slot = fsa::offender_slot(before, m_differ, lane);
            if (slot < FS_AUDIT_MAX_OFFENDERS)
                fsa::set_offender(R.offenders[slot], i, s);
        }
        if (lane == 0) {
            fsa::add_chunk(R, m_valid, m_differ, m_capped, m_stable);
            for (uint32_t j = 0; j < A.n_levels; j++)
                R.max_abs_diff[j] = level_max[j] > R.max_abs_diff[j] ? level_max[j] : R.max_abs_diff[j];
        }
        __syncthreads();
    }
    if (lane == 0)
        R.n_offenders = R.n_differ < FS_AUDIT_MAX_OFFENDERS ? R.n_differ : (uint32_t)FS_AUDIT_MAX_OFFENDERS;
    __syncthreads();
    for (uint32_t w = lane; w < sizeof(fs_audit_result) / 4; w += 64u)
        ((uint32_t *)A.out)[w] = ((const uint32_t *)&R)[w];
}

} // namespace

void fsk_exact_audit(const FsAuditArgs &A, hipStream_t s) { hipLaunchKernelGGL(k_exact_audit, dim3(1), dim3(64), 0, s, A); }
