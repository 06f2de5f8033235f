// tests/exact/exact_audit_host.cpp -- TEST INFRASTRUCTURE ONLY: csrc/exact_audit_math.hpp compiled for the host with g++.  The one
// wave of kernels_exact_audit.hip is a loop over 64 "lanes" here, its ballots are masks put together bit by bit and its butterfly
// maximum a plain one; classify, add_chunk, offender_slot, set_offender and level_diff are the kernel's own.
// tests/test_exact_audit_cpu.py compares the record with a numpy restatement.
#include <cstdint>
#include <cstring>

#include "../../fractalshark_amd/csrc/exact_audit_math.hpp"

extern "C" {

uint32_t exa_record_bytes(void) { return (uint32_t)sizeof(fs_audit_result); }

// counts[k * n + i] = run k of sample i; exact, frame, stable: per sample, as the kernel leaves them
void exa_audit(const void *iters, int iter_u64, uint32_t pitch, const uint32_t *xs, const uint32_t *ys, const uint64_t *counts,
               uint32_t n, uint32_t n_levels, uint64_t cap, fs_audit_result *out, uint64_t *exact, uint64_t *frame, uint32_t *stable)
{
    fs_audit_result R;
    memset(&R, 0, sizeof R);
    R.n_samples = n, R.n_levels = n_levels;
    for (uint32_t base = 0; base < n; base += 64u) {
        fsa::Sample s[64];
        uint64_t m_valid = 0, m_differ = 0, m_capped = 0, m_stable[FS_AUDIT_MAX_LEVELS] = {}, level_max[FS_AUDIT_MAX_LEVELS] = {};
        for (uint32_t lane = 0; lane < 64 && base + lane < n; lane++) {
            const uint32_t i = base + lane;
            s[lane] = fsa::classify(counts, n, n_levels, i, fsa::frame_at(iters, (uint32_t)iter_u64, pitch, xs[i], ys[i]), cap);
            exact[i] = s[lane].exact, frame[i] = s[lane].frame, stable[i] = s[lane].stable_bits;
            m_valid |= 1ull << lane;
            m_differ |= (uint64_t)s[lane].differ << lane;
            m_capped |= (uint64_t)s[lane].capped << lane;
            for (uint32_t j = 0; j < FS_AUDIT_MAX_LEVELS; j++) {
                m_stable[j] |= (uint64_t)((s[lane].stable_bits >> j) & 1u) << lane;
                const uint64_t d = fsa::level_diff(s[lane], j);
                level_max[j] = d > level_max[j] ? d : level_max[j];
            }
        }
        const uint32_t before = R.n_differ;
        for (uint32_t lane = 0; lane < 64; lane++)
            if ((m_differ >> lane) & 1ull) {
                const uint32_t slot = fsa::offender_slot(before, m_differ, lane);
                if (slot < FS_AUDIT_MAX_OFFENDERS)
                    fsa::set_offender(R.offenders[slot], base + lane, s[lane]);
            }
        fsa::add_chunk(R, m_valid, m_differ, m_capped, m_stable);
        for (uint32_t j = 0; j < n_levels; j++)
            R.max_abs_diff[j] = level_max[j] > R.max_abs_diff[j] ? level_max[j] : R.max_abs_diff[j];
    }
    R.n_offenders = R.n_differ < FS_AUDIT_MAX_OFFENDERS ? R.n_differ : (uint32_t)FS_AUDIT_MAX_OFFENDERS;
    *out = R;
}
}
