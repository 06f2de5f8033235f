// tests/exact/exact_wide_host.cpp -- TEST INFRASTRUCTURE ONLY: csrc/exact_wide_math.hpp compiled for the host with g++.  The wave of
// the wide exact kernel is a loop over 64 "lanes" here, and its ballots are masks put together bit by bit; the lane-local block
// functions and the carry look-ahead are the kernel's own.  tests/test_exact_wide_cpu.py compares them with Python integers.
// Every entry point that takes a block size returns -1 for one that is not instantiated.
#include <cstdint>
#include <cstring>

#include "../../fractalshark_amd/csrc/exact_wide_math.hpp"

namespace {

// out = a + b + cin over 64 blocks of M limbs, as wave_add of kernels_exact_wide.hip; returns the carry out
template <int M> int t_add(const uint32_t *a, const uint32_t *b, uint32_t cin, uint32_t *out)
{
    uint32_t s[64][M];
    uint64_t G = 0, P = 0;
    for (uint32_t t = 0; t < 64; t++) {
        uint32_t aa[M], bb[M];
        memcpy(aa, a + t * M, sizeof aa);
        memcpy(bb, b + t * M, sizeof bb);
        if (fsw::block_add<M>(aa, bb, s[t]))
            G |= 1ull << t;
        if (fsw::block_all_ones<M>(s[t]))
            P |= 1ull << t;
    }
    uint32_t cout = 0;
    const uint64_t C = fsw::carry_in_mask(G, P, cin, cout);
    for (uint32_t t = 0; t < 64; t++) {
        fsw::block_inc<M>(s[t], (uint32_t)(C >> t) & 1u);
        memcpy(out + t * M, s[t], sizeof s[t]);
    }
    return (int)cout;
}

// whether the 128-block s exceeds (reaches) R 2^2F, as wave_exceeds
template <int M> int t_exceeds(const uint32_t *s, const fsx::Params &P)
{
    uint64_t ne[2] = {0, 0}, gt[2] = {0, 0};
    for (uint32_t k = 0; k < 128; k++) {
        uint32_t blk[M];
        memcpy(blk, s + k * M, sizeof blk);
        const uint32_t c = fsw::block_compare<M>(blk, k * M, P);
        if (c != 0)
            ne[k / 64] |= 1ull << (k % 64);
        if (c == 1)
            gt[k / 64] |= 1ull << (k % 64);
    }
    return fsw::exceeds_from_masks(ne[1], gt[1], ne[0], gt[0], P.inclusive) ? 1 : 0;
}

} // namespace

#define DISPATCH(M_, CALL)                                                                                              \
    switch (M_) {                                                                                                       \
        FS_EXACT_WIDE_FOR_EACH_M(CALL)                                                                                  \
    default:                                                                                                            \
        return -1;                                                                                                      \
    }

extern "C" {

int exw_block_sizes(uint32_t *out, int cap)
{
    int n = 0;
#define ONE(M)                                                                                                          \
    if (n < cap)                                                                                                        \
        out[n++] = M;
    FS_EXACT_WIDE_FOR_EACH_M(ONE)
#undef ONE
    return n;
}

uint32_t exw_block_for(uint32_t limbs) { return fsw::block_for(limbs); }
uint32_t exw_max_limbs(void) { return fsw::kMaxLimbs; }

uint64_t exw_carry_in_mask(uint64_t G, uint64_t P, uint32_t cin, uint32_t *cout) { return fsw::carry_in_mask(G, P, cin, *cout); }

int exw_add(uint32_t M, const uint32_t *a, const uint32_t *b, uint32_t cin, uint32_t *out)
{
#define ONE(M)                                                                                                          \
    case M:                                                                                                             \
        return t_add<M>(a, b, cin, out);
    DISPATCH(M, ONE)
#undef ONE
}

int exw_exceeds(uint32_t M, const uint32_t *s, uint32_t frac_bits, uint32_t R, int inclusive)
{
    const fsx::Params P = fsx::make_params(frac_bits, R, inclusive);
#define ONE(M)                                                                                                          \
    case M:                                                                                                             \
        return t_exceeds<M>(s, P);
    DISPATCH(M, ONE)
#undef ONE
}
}
