// exact_wide_math.hpp -- the pieces of the wide exact kernel (kernels_exact_wide.hip) that do not need a wave: what one lane does to
// its block of M limbs, and the carry look-ahead that joins the 64 blocks.  Compiled by g++ too (tests/exact/exact_wide_host.cpp
// puts 64 "lanes" in a loop around them).
//
// A number of 64 M limbs is held as 64 blocks of M limbs, least significant block in lane 0.  An addition is done in every
// lane on its own block with carry-in 0; each lane then says whether its block GENERATES a carry (the block sum overflowed) and
// whether it PROPAGATES one (the block sum is all ones: a carry coming in would go out again).  The two 64-bit masks G and P
// decide the carry into every block in one 64-bit addition: add the numbers a = G | P and b = G.  Bit t of them is (1, 1) where
// the block generates, (1, 0) where it propagates and (0, 0) where it does neither, so the binary adder's carry into bit t is
// the carry into block t, and a sum bit s_t = a_t ^ b_t ^ carry_t gives it back: carry = (a + b + cin) ^ P.  A block cannot do
// both -- a block sum that overflowed is at most 2^(32M) - 2 -- and where a caller sets both, G wins.
#ifndef FS_EXACT_WIDE_MATH_HPP
#define FS_EXACT_WIDE_MATH_HPP

#include "exact_math.hpp"

// every instantiated block size: 64 M limbs, frac_bits up to 32 * 704 - 10 = 22518
#define FS_EXACT_WIDE_FOR_EACH_M(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11)

namespace fsw {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kMinLimbs = 2, kMaxLimbs = 704, kMaxBlock = 11;

// limbs per lane for a limb count
constexpr uint32_t block_for(uint32_t limbs) { return (limbs + kLanes - 1) / kLanes; }

// bit t = the carry into block t; cout = the carry out of block 63
FSX_HD uint64_t carry_in_mask(uint64_t G, uint64_t P, uint32_t cin, uint32_t &cout)
{
    P &= ~G;
    const uint64_t a = G | P;
    uint64_t s, t;
    const uint32_t c1 = __builtin_add_overflow(a, G, &s) ? 1u : 0u;
    const uint32_t c2 = __builtin_add_overflow(s, (uint64_t)cin, &t) ? 1u : 0u;
    cout = c1 | c2;
    return t ^ P;
}

// s = a + b on one block, carry-in 0; returns the carry out
template <int M> FSX_HD uint32_t block_add(const uint32_t (&a)[M], const uint32_t (&b)[M], uint32_t (&s)[M])
{
    uint32_t c = 0;
    FSX_UNROLL
    for (int i = 0; i < M; i++)
        s[i] = fsx::addc(a[i], b[i], c);
    return c;
}

template <int M> FSX_HD bool block_all_ones(const uint32_t (&s)[M])
{
    uint32_t all = ~0u;
    FSX_UNROLL
    for (int i = 0; i < M; i++)
        all &= s[i];
    return all == ~0u;
}

// The device compiler must not look through `x` (no instruction is emitted).  See block_inc.
#if defined(__HIP_DEVICE_COMPILE__)
#define FSW_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define FSW_OPAQUE(x) ((void)0)
#endif

// s += c (c = 0 or 1), wrapping: the carry out of an all-ones block is already in the look-ahead, so the last limb's carry is
// dropped on purpose.  That leaves the last limb a plain `add x, carry`, and the gfx950 back end folds a carry chain over constant
// zeros that follows it, (uaddo_carry (add x, y), 0, c) -> (uaddo_carry x, y, c), into one instruction whose carry-out is then the
// dropped carry as well: every block that wrapped to zero would generate a carry a second time (DESIGN.md 6.3 "Wide").  The last
// limb is therefore handed on as a value the compiler knows nothing about.
template <int M> FSX_HD void block_inc(uint32_t (&s)[M], uint32_t c)
{
    FSX_UNROLL
    for (int i = 0; i < M; i++)
        s[i] = fsx::addc(s[i], 0u, c);
    FSW_OPAQUE(s[M - 1]);
}

// How a block compares with the same block of the bailout value R 2^2F, whose only non-zero limbs are bail_q and bail_q + 1:
// 0 equal, 1 greater, 2 less.  first = the index of the block's limb 0 in the whole number.
template <int M> FSX_HD uint32_t block_compare(const uint32_t (&s)[M], uint32_t first, const fsx::Params &P)
{
    uint32_t res = 0;
    FSX_UNROLL
    for (int i = 0; i < M; i++) { // from the low limb up: a higher limb that differs overrides
        const uint32_t g = first + (uint32_t)i;
        const uint32_t b = g == P.bail_q ? P.bail_lo : (g == P.bail_q + 1 ? P.bail_hi : 0u);
        res = s[i] > b ? 1u : (s[i] < b ? 2u : res);
    }
    return res;
}

// the highest block that differs decides: NE = blocks that differ, GT = blocks that are greater
FSX_HD bool exceeds_from_masks(uint64_t ne_hi, uint64_t gt_hi, uint64_t ne_lo, uint64_t gt_lo, uint32_t inclusive)
{
    if (ne_hi)
        return (gt_hi >> (63 - __builtin_clzll(ne_hi))) & 1u;
    if (ne_lo)
        return (gt_lo >> (63 - __builtin_clzll(ne_lo))) & 1u;
    return inclusive != 0;
}

// The period rule of the wide point runs (kernels_exact_wide.hip, the P = true instantiations) compares two unsigned numbers of
// 128 blocks the same way.  How block a compares with block b: 0 equal, 1 greater, 2 less.
template <int M> FSX_HD uint32_t block_order(const uint32_t (&a)[M], const uint32_t (&b)[M])
{
    uint32_t res = 0;
    FSX_UNROLL
    for (int i = 0; i < M; i++) // from the low limb up: a higher limb that differs overrides
        res = a[i] > b[i] ? 1u : (a[i] < b[i] ? 2u : res);
    return res;
}

// strictly less -- false on equality: NE = blocks that differ, LT = blocks that are less; the highest block that differs decides
FSX_HD bool less_from_masks(uint64_t ne_hi, uint64_t lt_hi, uint64_t ne_lo, uint64_t lt_lo)
{
    if (ne_hi)
        return (lt_hi >> (63 - __builtin_clzll(ne_hi))) & 1u;
    if (ne_lo)
        return (lt_lo >> (63 - __builtin_clzll(ne_lo))) & 1u;
    return false;
}

} // namespace fsw

#endif
