// tests/truth/exact_counts.cpp -- TEST INFRASTRUCTURE ONLY: exact Mandelbrot escape counts from GMP integer iteration.
//
// The plain high-precision statement of what every render path of this project computes: for a sample's c, the first
// n >= 1 with |z_n|^2 > R (or >= R) under z_0 = 0, z_{n+1} = z_n^2 + c.  It shares nothing with oracle/ or the product:
// no header of either is included, and no floating-point number takes part.
//
//   * The view's bounding box arrives as the decimal strings View.bbox() gives ("-5.48...e-01"); each is read as an exact
//     rational.  c = (minX + x * (maxX - minX) / w, maxY - y * (maxY - minY) / h), exactly, then floored to frac_bits
//     fractional bits.  (The map the reference's CPU paths imply: dx = (maxX - minX) / (width * AA), centerX = orbitX - minX,
//     deltaReal = dx * x - centerX, deltaImaginary = -dy * y - (orbitY - maxY); Fractal.cpp:2230-2238, 2269-2275.)
//   * z is iterated in fixed point on mpz_t: x' = floor((x^2 - y^2) / 2^F) + cx, y' = floor(2xy / 2^F) + cy.  The escape test
//     compares the untruncated x^2 + y^2 with R * 2^2F.
//   * For each shift k the count is recomputed at c + s, c - s, c + is, c - is with s = (maxX - minX) / 2^k (a fraction of
//     the frame width, the same length on both axes); stable[i * n_shifts + j] = 1 when all four equal the count at c.
//
// counts[i] = the first such n <= limit, or 0 when there is none.
#include <gmp.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace {

// "[-]d.ddddde[+-]XX" (or plain "[-]ddd.ddd") -> exact rational
bool parse_decimal(const char *s, mpq_t out)
{
    std::string digits;
    bool neg = false, seen_point = false;
    long frac = 0, exp10 = 0;
    const char *p = s;
    if (*p == '-' || *p == '+')
        neg = *p++ == '-';
    for (; *p; p++) {
        if (*p >= '0' && *p <= '9') {
            digits.push_back(*p);
            if (seen_point)
                frac++;
        } else if (*p == '.' && !seen_point) {
            seen_point = true;
        } else if (*p == 'e' || *p == 'E') {
            char *end = nullptr;
            exp10 = strtol(p + 1, &end, 10);
            if (end == p + 1 || *end)
                return false;
            break;
        } else {
            return false;
        }
    }
    if (digits.empty())
        return false;
    mpz_t num, pow;
    mpz_init(num);
    mpz_init(pow);
    mpz_set_str(num, digits.c_str(), 10);
    if (neg)
        mpz_neg(num, num);
    const long e = exp10 - frac;
    mpz_ui_pow_ui(pow, 10, (unsigned long)(e < 0 ? -e : e));
    mpq_set_z(out, num);
    mpq_t q;
    mpq_init(q);
    mpq_set_z(q, pow);
    if (e < 0)
        mpq_div(out, out, q);
    else
        mpq_mul(out, out, q);
    mpq_clear(q);
    mpz_clear(num);
    mpz_clear(pow);
    return true;
}

// floor(q * 2^F)
void to_fixed(mpz_t out, const mpq_t q, unsigned F)
{
    mpz_mul_2exp(out, mpq_numref(q), F);
    mpz_fdiv_q(out, out, mpq_denref(q));
}

struct Iterator {
    mpz_t x, y, x2, y2, s, t, bail;
    unsigned F;
    bool inclusive;
    Iterator(unsigned F_, const mpq_t R, bool inclusive_) : F(F_), inclusive(inclusive_)
    {
        mpz_inits(x, y, x2, y2, s, t, bail, nullptr);
        to_fixed(bail, R, 2 * F);
    }
    ~Iterator() { mpz_clears(x, y, x2, y2, s, t, bail, nullptr); }
    uint64_t count(const mpz_t cx, const mpz_t cy, uint64_t limit)
    {
        mpz_set(x, cx); // z_1 = c
        mpz_set(y, cy);
        for (uint64_t n = 1; n <= limit; n++) {
            mpz_mul(x2, x, x);
            mpz_mul(y2, y, y);
            mpz_add(s, x2, y2);
            const int c = mpz_cmp(s, bail);
            if (c > 0 || (inclusive && c == 0))
                return n;
            mpz_mul(t, x, y);
            mpz_mul_2exp(t, t, 1);
            mpz_fdiv_q_2exp(t, t, F);
            mpz_add(y, t, cy);
            mpz_sub(s, x2, y2);
            mpz_fdiv_q_2exp(s, s, F);
            mpz_add(x, s, cx);
        }
        return 0;
    }
};

} // namespace

// bbox = {minX, minY, maxX, maxY}; w, h = the frame in samples (width x AA, height x AA); R = r_num / r_den;
// inclusive: 0 = escape when |z|^2 > R, 1 = when |z|^2 >= R.  Returns 0, or -1 on a string it cannot read.
extern "C" int exc_exact_counts(const char *const bbox[4], uint32_t w, uint32_t h, const uint32_t *xs, const uint32_t *ys,
                                uint64_t n_samples, uint64_t limit, uint32_t r_num, uint32_t r_den, int inclusive,
                                uint32_t frac_bits, const int32_t *shifts, int n_shifts, uint64_t *counts, uint8_t *stable,
                                int threads)
{
    mpq_t b[4], spanx, spany, R;
    for (auto &q : b)
        mpq_init(q);
    mpq_inits(spanx, spany, R, nullptr);
    bool ok = true;
    for (int i = 0; i < 4; i++)
        ok = ok && parse_decimal(bbox[i], b[i]);
    if (!ok) {
        for (auto &q : b)
            mpq_clear(q);
        mpq_clears(spanx, spany, R, nullptr);
        return -1;
    }
    mpq_sub(spanx, b[2], b[0]);
    mpq_sub(spany, b[3], b[1]);
    mpq_set_ui(R, r_num, r_den);
    mpq_canonicalize(R);
    if (threads < 1)
        threads = 1;
    if (threads > 16)
        threads = 16;
    std::atomic<uint64_t> next{0};
    auto work = [&]() {
        Iterator it(frac_bits, R, inclusive != 0);
        mpq_t cx, cy, q, sh;
        mpz_t fx, fy;
        mpq_inits(cx, cy, q, sh, nullptr);
        mpz_inits(fx, fy, nullptr);
        for (;;) {
            const uint64_t i = next.fetch_add(1);
            if (i >= n_samples)
                break;
            mpq_set_ui(q, xs[i], w);
            mpq_canonicalize(q);
            mpq_mul(cx, spanx, q);
            mpq_add(cx, cx, b[0]);
            mpq_set_ui(q, ys[i], h);
            mpq_canonicalize(q);
            mpq_mul(cy, spany, q);
            mpq_sub(cy, b[3], cy);
            to_fixed(fx, cx, frac_bits);
            to_fixed(fy, cy, frac_bits);
            const uint64_t base = it.count(fx, fy, limit);
            counts[i] = base;
            for (int j = 0; j < n_shifts; j++) {
                mpq_set(sh, spanx);
                mpq_div_2exp(sh, sh, (mp_bitcnt_t)shifts[j]);
                bool same = true;
                for (int d = 0; d < 4 && same; d++) {
                    mpq_set(q, d < 2 ? cx : cy);
                    if (d & 1)
                        mpq_sub(q, q, sh);
                    else
                        mpq_add(q, q, sh);
                    if (d < 2) {
                        to_fixed(fx, q, frac_bits);
                        to_fixed(fy, cy, frac_bits);
                    } else {
                        to_fixed(fx, cx, frac_bits);
                        to_fixed(fy, q, frac_bits);
                    }
                    same = it.count(fx, fy, limit) == base;
                }
                stable[i * (uint64_t)n_shifts + j] = same ? 1 : 0;
            }
        }
        mpq_clears(cx, cy, q, sh, nullptr);
        mpz_clears(fx, fy, nullptr);
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back(work);
    for (auto &t : pool)
        t.join();
    for (auto &q : b)
        mpq_clear(q);
    mpq_clears(spanx, spany, R, nullptr);
    return 0;
}
