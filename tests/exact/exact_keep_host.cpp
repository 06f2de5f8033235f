// tests/exact/exact_keep_host.cpp -- TEST INFRASTRUCTURE ONLY: the park-and-resume rule of csrc/exact_cycle_math.hpp (fs_set_exact_keep,
// fs_render_exact_continue) compiled for the host with g++, as a program of its own: every sample runs from z_1 = c to the cap N1,
// and one that ends capped there is parked and resumed to the cap N2.  tests/test_exact_keep_cpu.py compares what it prints with
// the Python model run straight to N2.
//
// stdin:   limbs frac_bits R inclusive N1 N2 fp_bits check n
//          then n lines of 2 * limbs hexadecimal words: cx (low limb first), then cy
// stdout:  per sample  outcome1 value1 steps1 compares1  outcome2 value2 steps2 compares2  n_parked
//          (outcome: 0 escaped, 1 capped, 2 proved; the second run is "1 N2 0 0" -- nothing happened -- when the first did not end
//          capped, n_parked the n the parked sample held, else 0)
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../fractalshark_amd/csrc/exact_cycle_math.hpp"

namespace {

struct Job {
    uint32_t limbs, frac_bits, R, fp_bits;
    int inclusive, check;
    uint64_t n1, n2;
};

template <int L> void run_one(const Job &J, const uint32_t *c)
{
    uint32_t cx[L], cy[L], mx, my;
    for (int i = 0; i < L; i++)
        cx[i] = c[i], cy[i] = c[L + i];
    fsx::cycle_masks(J.fp_bits, mx, my);
    const fsx::Params P = fsx::make_params(J.frac_bits, J.R, J.inclusive);
    fsx::CycleState<L> S;
    const fsx::CycleRun a = fsx::cycle_run_from<L>(S, false, cx, cy, P, J.n1, J.check != 0, mx, my);
    fsx::CycleRun b{fsx::kCycleCapped, J.n2, 0, 0};
    uint64_t parked_n = 0;
    if (a.outcome == fsx::kCycleCapped && J.n2 > J.n1) {
        parked_n = S.n;
        b = fsx::cycle_run_from<L>(S, true, cx, cy, P, J.n2, J.check != 0, mx, my);
    }
    printf("%u %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", a.outcome, a.value, a.steps,
           a.compares, b.outcome, b.value, b.steps, b.compares, parked_n);
}

} // namespace

int main()
{
    Job J{};
    uint64_t n = 0;
    if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %d %" SCNu64 " %" SCNu64 " %" SCNu32 " %d %" SCNu64, &J.limbs, &J.frac_bits, &J.R,
              &J.inclusive, &J.n1, &J.n2, &J.fp_bits, &J.check, &n) != 9)
        return 2;
    if (J.limbs < fsx::kMinLimbs || J.limbs > fsx::kMaxLimbs)
        return 3;
    std::vector<uint32_t> c(2 * J.limbs);
    for (uint64_t i = 0; i < n; i++) {
        for (uint32_t k = 0; k < 2 * J.limbs; k++)
            if (scanf("%" SCNx32, &c[k]) != 1)
                return 4;
        switch (J.limbs) {
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        run_one<L>(J, c.data());                                                                                       \
        break;
            FS_EXACT_FOR_EACH_L(ONE)
#undef ONE
        }
    }
    return 0;
}
