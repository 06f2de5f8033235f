// exact_audit_math.hpp -- the rule of fs_exact_audit, one text for the device (kernels_exact_audit.hip) and for the host (g++;
// tests/exact/exact_audit_host.cpp walks the samples with the same functions, its wave a loop over 64 lanes).
//
// A sample has 1 + 4 n_levels runs of the exact recurrence: run 0 at c, run 1 + 4 j + d at c + s_j, c - s_j, c + i s_j, c - i s_j.
// counts[k * n_samples + i] is run k of sample i.  Per sample (classify):
//     exact        = the count of run 0
//     stable_bits  : bit j set when the four counts of level j equal exact
//     differ       = frame != exact,   capped = exact == n_iterations,   abs_diff = |frame - exact|
// The record (fs_audit_result, fs_layout.h) is built 64 samples at a time, in index order.  What a chunk adds is a function of
// masks over its lanes -- the ballots of the kernel -- so the sums are popcounts, an offender's place is a prefix count, and no
// result depends on the order in which anything ran.
#ifndef FS_EXACT_AUDIT_MATH_HPP
#define FS_EXACT_AUDIT_MATH_HPP

#include <stddef.h>
#include <stdint.h>

#include "../../include/fs_layout.h"

#if defined(__HIPCC__)
#define FSA_HD __host__ __device__ inline
#else
#define FSA_HD inline
#endif

namespace fsa {

struct Sample {
    uint64_t exact, frame, abs_diff;
    uint32_t stable_bits;
    bool differ, capped;
};

// the frame's value at (x, y); pitch in elements
FSA_HD uint64_t frame_at(const void *iters, uint32_t iter_u64, uint32_t pitch, uint32_t x, uint32_t y)
{
    const size_t idx = (size_t)y * pitch + x;
    return iter_u64 ? ((const uint64_t *)iters)[idx] : (uint64_t)((const uint32_t *)iters)[idx];
}

FSA_HD Sample classify(const uint64_t *counts, uint32_t n_samples, uint32_t n_levels, uint32_t i, uint64_t frame, uint64_t cap)
{
    Sample s;
    s.exact = counts[i];
    s.frame = frame;
    s.stable_bits = 0;
    for (uint32_t j = 0; j < n_levels; j++) {
        bool same = true;
        for (uint32_t d = 0; d < 4; d++)
            same = same && counts[(size_t)(1 + 4 * j + d) * n_samples + i] == s.exact;
        s.stable_bits |= (same ? 1u : 0u) << j;
    }
    s.differ = frame != s.exact;
    s.capped = s.exact == cap;
    s.abs_diff = frame > s.exact ? frame - s.exact : s.exact - frame;
    return s;
}

FSA_HD uint32_t popc(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// What one chunk adds to the counts of the record.  valid, differ, capped, stable[j]: masks over the chunk's lanes (differ, capped
// and stable[] inside valid).
FSA_HD void add_chunk(fs_audit_result &R, uint64_t valid, uint64_t differ, uint64_t capped, const uint64_t *stable)
{
    R.n_differ += popc(differ);
    R.n_equal += popc(valid & ~differ);
    R.n_capped += popc(capped);
    for (uint32_t j = 0; j < R.n_levels; j++) {
        R.stable[j] += popc(stable[j]);
        R.stable_differ[j] += popc(stable[j] & differ);
        R.stable_capped[j] += popc(stable[j] & capped);
    }
}

// The place of lane's sample among the offenders, `before` differing samples having come in earlier chunks; recorded when below
// FS_AUDIT_MAX_OFFENDERS.
FSA_HD uint32_t offender_slot(uint32_t before, uint64_t differ, uint32_t lane) { return before + popc(differ & ((1ull << lane) - 1ull)); }

FSA_HD void set_offender(fs_audit_offender &o, uint32_t i, const Sample &s)
{
    o.sample = i, o.stable_bits = s.stable_bits;
    o.frame_value = s.frame, o.exact_value = s.exact;
}

// what a sample offers to max_abs_diff[j]: its difference where it is stable at the level and differs, else 0
FSA_HD uint64_t level_diff(const Sample &s, uint32_t j) { return s.differ && ((s.stable_bits >> j) & 1u) ? s.abs_diff : 0ull; }

} // namespace fsa

#endif
