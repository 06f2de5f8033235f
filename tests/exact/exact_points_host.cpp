// tests/exact/exact_points_host.cpp -- TEST INFRASTRUCTURE ONLY: csrc/exact_atom_math.hpp compiled for the host with g++: the point
// runs of fs_exact_eval_points (fsx::point_run), one run after another.  tests/test_exact_points_cpu.py compares it with Python
// integers.
#include <cstdint>
#include <cstring>

#include "../../fractalshark_amd/csrc/exact_atom_math.hpp"

namespace {

template <int L>
fsx::PointRun t_run(const uint32_t *cx, const uint32_t *cy, const fsx::Params &P, uint64_t len, uint32_t shift, uint32_t *end)
{
    uint32_t a[L], b[L], e[2 * L];
    memcpy(a, cx, sizeof a);
    memcpy(b, cy, sizeof b);
    const fsx::PointRun r = fsx::point_run<L>(a, b, P, len, shift, e);
    memcpy(end, e, sizeof e);
    return r;
}

} // namespace

// The n runs (cx[i], cy[i]) (limbs limbs each, run-major) of lengths len[i]: out[3 * i ..] = value, atom period, steps;
// end[2 * limbs * i ..] = the limbs of x_len, then of y_len (all zero when the run is short of its length).  key_bits:
// fs_set_exact_atom_key_bits.  -1: limb count not instantiated.
extern "C" int exp_point_runs(uint32_t limbs, uint64_t n, const uint32_t *cx, const uint32_t *cy, const uint64_t *len, uint32_t frac_bits,
                              uint32_t R, int inclusive, uint32_t key_bits, uint64_t *out, uint32_t *end)
{
    const fsx::Params P = fsx::make_params(frac_bits, R, inclusive);
    if (limbs < fsx::kMinLimbs || limbs > fsx::kMaxLimbs)
        return -1;
    const uint32_t shift = fsx::atom_key_shift(key_bits);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t *a = cx + i * limbs, *b = cy + i * limbs;
        uint32_t *e = end + 2 * i * limbs;
        fsx::PointRun r{};
        switch (limbs) {
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        r = t_run<L>(a, b, P, len[i], shift, e);                                                                       \
        break;
            FS_EXACT_FOR_EACH_L(ONE)
#undef ONE
        }
        out[3 * i] = r.value, out[3 * i + 1] = r.atom, out[3 * i + 2] = r.steps;
    }
    return 0;
}
