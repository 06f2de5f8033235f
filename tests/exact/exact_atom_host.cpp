// tests/exact/exact_atom_host.cpp -- TEST INFRASTRUCTURE ONLY: csrc/exact_atom_math.hpp compiled for the host with g++: the exact
// renderer's step loop with the period planes' rule, one sample after another.  tests/test_exact_atom_cpu.py compares it with Python
// integers.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../fractalshark_amd/csrc/exact_atom_math.hpp"

namespace {

template <int L>
fsx::AtomRun t_run(const uint32_t *cx, const uint32_t *cy, const fsx::Params &P, uint64_t cap, bool check, uint32_t mx, uint32_t my,
                   uint32_t shift)
{
    uint32_t a[L], b[L];
    memcpy(a, cx, sizeof a);
    memcpy(b, cy, sizeof b);
    return fsx::atom_run<L>(a, b, P, cap, check, mx, my, shift);
}

} // namespace

// The n samples (cx[i], cy[i]) (limbs limbs each, sample-major) from z_1 = c to their end, with the cycle check (check != 0) or
// without: out[7 * i ..] = outcome (0 escaped, 1 capped, 2 proved), value, atom period, proof index, cycle length, steps, times the
// minimum was read back.  key_bits: fs_set_exact_atom_key_bits.  -1: limb count not instantiated.
extern "C" int exa_atom_runs(uint32_t limbs, uint64_t n, const uint32_t *cx, const uint32_t *cy, uint32_t frac_bits, uint32_t R,
                             int inclusive, uint64_t cap, int check, uint32_t key_bits, uint64_t *out, int threads)
{
    const fsx::Params P = fsx::make_params(frac_bits, R, inclusive);
    if (limbs < fsx::kMinLimbs || limbs > fsx::kMaxLimbs)
        return -1;
    uint32_t mx, my;
    fsx::cycle_masks(0, mx, my);
    const uint32_t shift = fsx::atom_key_shift(key_bits);
    std::atomic<uint64_t> next{0};
    auto work = [&]() {
        for (;;) {
            const uint64_t i = next.fetch_add(1);
            if (i >= n)
                break;
            const uint32_t *a = cx + i * limbs, *b = cy + i * limbs;
            fsx::AtomRun r{};
            switch (limbs) {
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        r = t_run<L>(a, b, P, cap, check != 0, mx, my, shift);                                                         \
        break;
                FS_EXACT_FOR_EACH_L(ONE)
#undef ONE
            }
            uint64_t *o = out + 7 * i;
            o[0] = r.outcome, o[1] = r.value, o[2] = r.atom, o[3] = r.proof_n, o[4] = r.cyclen, o[5] = r.steps, o[6] = r.compares;
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

// the key of an unsigned number of 8 limbs (tests of the key's order)
extern "C" uint64_t exa_atom_key8(const uint32_t *w, uint32_t key_bits)
{
    uint32_t a[8];
    memcpy(a, w, sizeof a);
    return fsx::atom_key<8>(a, fsx::atom_key_shift(key_bits));
}
