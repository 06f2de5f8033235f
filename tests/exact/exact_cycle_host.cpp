// tests/exact/exact_cycle_host.cpp -- TEST INFRASTRUCTURE ONLY: csrc/exact_cycle_math.hpp compiled for the host with g++: the exact
// renderer's step loop with the cycle check, one sample after another.  tests/test_exact_cycle_cpu.py compares it with Python
// integers.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../fractalshark_amd/csrc/exact_cycle_math.hpp"

namespace {

template <int L> fsx::CycleRun t_run(const uint32_t *cx, const uint32_t *cy, const fsx::Params &P, uint64_t cap, uint32_t mx, uint32_t my)
{
    uint32_t a[L], b[L];
    memcpy(a, cx, sizeof a);
    memcpy(b, cy, sizeof b);
    return fsx::cycle_run<L>(a, b, P, cap, mx, my);
}

} // namespace

// The n samples (cx[i], cy[i]) (limbs limbs each, sample-major) from z_1 = c to their end: outcome[i] (0 escaped, 1 capped, 2
// proved), value[i], steps[i] and compares[i].  fp_bits: fs_set_exact_cycle_fingerprint_bits.  -1: limb count not instantiated.
extern "C" int exc_cycle_runs(uint32_t limbs, uint64_t n, const uint32_t *cx, const uint32_t *cy, uint32_t frac_bits, uint32_t R,
                              int inclusive, uint64_t cap, uint32_t fp_bits, uint32_t *outcome, uint64_t *value, uint64_t *steps,
                              uint64_t *compares, int threads)
{
    const fsx::Params P = fsx::make_params(frac_bits, R, inclusive);
    if (limbs < fsx::kMinLimbs || limbs > fsx::kMaxLimbs)
        return -1;
    uint32_t mx, my;
    fsx::cycle_masks(fp_bits, mx, my);
    std::atomic<uint64_t> next{0};
    auto work = [&]() {
        for (;;) {
            const uint64_t i = next.fetch_add(1);
            if (i >= n)
                break;
            const uint32_t *a = cx + i * limbs, *b = cy + i * limbs;
            fsx::CycleRun r{};
            switch (limbs) {
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        r = t_run<L>(a, b, P, cap, mx, my);                                                                            \
        break;
                FS_EXACT_FOR_EACH_L(ONE)
#undef ONE
            }
            outcome[i] = r.outcome, value[i] = r.value, steps[i] = r.steps, compares[i] = r.compares;
        }
    };
    if (threads < 1)
        threads = 1;
    if (threads > 16)
        threads = 16;
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back(work);
    for (auto &t : pool)
        t.join();
    return 0;
}
