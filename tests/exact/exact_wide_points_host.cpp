// tests/exact/exact_wide_points_host.cpp -- TEST INFRASTRUCTURE ONLY: the period rule's compare of the wide point-run kernels
// (csrc/exact_wide_math.hpp: block_order, less_from_masks) compiled for the host with g++.  The wave is a loop over 64 "lanes" and
// its four ballots are masks put together bit by bit, as in exact_wide_host.cpp; tests/test_exact_wide_points_cpu.py compares the
// answers with Python integers.  Every entry point returns -1 for a block size that is not instantiated.
#include <cstdint>
#include <cstring>

#include "../../fractalshark_amd/csrc/exact_wide_math.hpp"

namespace {

// whether the 128-block a is strictly below the 128-block b, as wave_below of kernels_exact_wide.hip: lane t compares blocks t
// and 64 + t
template <int M> int t_below(const uint32_t *a, const uint32_t *b)
{
    uint64_t ne[2] = {0, 0}, lt[2] = {0, 0};
    for (uint32_t t = 0; t < 64; t++)
        for (uint32_t half = 0; half < 2; half++) {
            uint32_t aa[M], bb[M];
            memcpy(aa, a + (64 * half + t) * M, sizeof aa);
            memcpy(bb, b + (64 * half + t) * M, sizeof bb);
            const uint32_t c = fsw::block_order<M>(aa, bb);
            if (c != 0)
                ne[half] |= 1ull << t;
            if (c == 2)
                lt[half] |= 1ull << t;
        }
    return fsw::less_from_masks(ne[1], lt[1], ne[0], lt[0]) ? 1 : 0;
}

// block_order of one pair of blocks
template <int M> int t_order(const uint32_t *a, const uint32_t *b)
{
    uint32_t aa[M], bb[M];
    memcpy(aa, a, sizeof aa);
    memcpy(bb, b, sizeof bb);
    return (int)fsw::block_order<M>(aa, bb);
}

} // namespace

#define DISPATCH(M_, CALL)                                                                                              \
    switch (M_) {                                                                                                       \
        FS_EXACT_WIDE_FOR_EACH_M(CALL)                                                                                  \
    default:                                                                                                            \
        return -1;                                                                                                      \
    }

extern "C" {

int exwp_below(uint32_t M, const uint32_t *a, const uint32_t *b)
{
#define ONE(M)                                                                                                          \
    case M:                                                                                                             \
        return t_below<M>(a, b);
    DISPATCH(M, ONE)
#undef ONE
}

int exwp_block_order(uint32_t M, const uint32_t *a, const uint32_t *b)
{
#define ONE(M)                                                                                                          \
    case M:                                                                                                             \
        return t_order<M>(a, b);
    DISPATCH(M, ONE)
#undef ONE
}

int exwp_less_from_masks(uint64_t ne_hi, uint64_t lt_hi, uint64_t ne_lo, uint64_t lt_lo)
{
    return fsw::less_from_masks(ne_hi, lt_hi, ne_lo, lt_lo) ? 1 : 0;
}
}
