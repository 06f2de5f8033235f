// tests/exact/exact_host.cpp -- TEST INFRASTRUCTURE ONLY: csrc/exact_math.hpp compiled for the host with g++, one C entry point per
// function, dispatched over every instantiated limb count.  tests/test_exact_math_cpu.py compares them with Python integers.
// Every entry point returns -1 for a limb count that is not instantiated.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../fractalshark_amd/csrc/exact_math.hpp"

namespace {

template <int L> void t_square(const uint32_t *a, uint32_t *p)
{
    uint32_t aa[L], pp[2 * L];
    memcpy(aa, a, sizeof aa);
    fsx::square<L>(aa, pp);
    memcpy(p, pp, sizeof pp);
}

template <int L> void t_mul(const uint32_t *a, const uint32_t *b, uint32_t *p)
{
    uint32_t aa[L], bb[L], pp[2 * L];
    memcpy(aa, a, sizeof aa);
    memcpy(bb, b, sizeof bb);
    fsx::mul<L>(aa, bb, pp);
    memcpy(p, pp, sizeof pp);
}

template <int L> void t_shift(const uint32_t *d, const fsx::Params &P, uint32_t *out)
{
    uint32_t dd[2 * L], oo[L];
    memcpy(dd, d, sizeof dd);
    fsx::shift_floor<L>(dd, P, oo);
    memcpy(out, oo, sizeof oo);
}

template <int L> int t_exceeds(const uint32_t *s, const fsx::Params &P)
{
    uint32_t ss[2 * L];
    memcpy(ss, s, sizeof ss);
    return fsx::exceeds<L>(ss, P) ? 1 : 0;
}

template <int L> int t_magnitude(const uint32_t *x, uint32_t *out)
{
    uint32_t xx[L], oo[L];
    memcpy(xx, x, sizeof xx);
    const int neg = (int)fsx::magnitude<L>(xx, oo);
    memcpy(out, oo, sizeof oo);
    return neg;
}

template <int L> uint64_t t_count(const uint32_t *cx, const uint32_t *cy, const fsx::Params &P, uint64_t limit)
{
    uint32_t a[L], b[L];
    memcpy(a, cx, sizeof a);
    memcpy(b, cy, sizeof b);
    return fsx::count<L>(a, b, P, limit);
}

} // namespace

#define DISPATCH(expr)                                                                                                 \
    switch (limbs) {                                                                                                   \
        FS_EXACT_FOR_EACH_L(expr)                                                                                      \
    default:                                                                                                           \
        return -1;                                                                                                     \
    }

extern "C" int exh_limb_counts(uint32_t *out, int cap)
{
    int n = 0;
#define ONE(L)                                                                                                         \
    if (n < cap)                                                                                                       \
        out[n] = L;                                                                                                    \
    n++;
    FS_EXACT_FOR_EACH_L(ONE)
#undef ONE
    return n;
}

extern "C" int exh_square(uint32_t limbs, const uint32_t *a, uint32_t *p)
{
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        t_square<L>(a, p);                                                                                             \
        return 0;
    DISPATCH(ONE)
#undef ONE
}

extern "C" int exh_mul(uint32_t limbs, const uint32_t *a, const uint32_t *b, uint32_t *p)
{
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        t_mul<L>(a, b, p);                                                                                             \
        return 0;
    DISPATCH(ONE)
#undef ONE
}

extern "C" int exh_magnitude(uint32_t limbs, const uint32_t *x, uint32_t *out)
{
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        return t_magnitude<L>(x, out);
    DISPATCH(ONE)
#undef ONE
}

// d: 2 * limbs limbs, two's complement; out = floor(d / 2^frac_bits), limbs limbs
extern "C" int exh_shift_floor(uint32_t limbs, const uint32_t *d, uint32_t frac_bits, uint32_t *out)
{
    const fsx::Params P = fsx::make_params(frac_bits, 4, 0);
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        t_shift<L>(d, P, out);                                                                                         \
        return 0;
    DISPATCH(ONE)
#undef ONE
}

// 1 when the unsigned 2 * limbs-limb s is above (inclusive: at or above) R * 2^(2 frac_bits)
extern "C" int exh_exceeds(uint32_t limbs, const uint32_t *s, uint32_t frac_bits, uint32_t R, int inclusive)
{
    const fsx::Params P = fsx::make_params(frac_bits, R, inclusive);
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        return t_exceeds<L>(s, P);
    DISPATCH(ONE)
#undef ONE
}

// counts[i] for the n samples (cx[i], cy[i]) (limbs limbs each, sample-major): the first step <= limit that escapes, 0 = none
extern "C" int exh_counts(uint32_t limbs, uint64_t n, const uint32_t *cx, const uint32_t *cy, uint32_t frac_bits, uint32_t R,
                          int inclusive, uint64_t limit, uint64_t *counts, int threads)
{
    const fsx::Params P = fsx::make_params(frac_bits, R, inclusive);
    if (limbs < fsx::kMinLimbs || limbs > fsx::kMaxLimbs)
        return -1;
    std::atomic<uint64_t> next{0};
    auto work = [&]() {
        for (;;) {
            const uint64_t i = next.fetch_add(1);
            if (i >= n)
                break;
            const uint32_t *a = cx + i * limbs, *b = cy + i * limbs;
            switch (limbs) {
#define ONE(L)                                                                                                         \
    case L:                                                                                                            \
        counts[i] = t_count<L>(a, b, P, limit);                                                                        \
        break;
                FS_EXACT_FOR_EACH_L(ONE)
#undef ONE
            }
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
