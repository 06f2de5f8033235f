// exact_atom_math.hpp -- the exact renderer's period planes (DESIGN.md 6.3 "Period planes"; fs_set_exact_periods), for the device
// (kernels_exact.hip, the P = true instantiations) and for the host (g++; tests/exact/exact_atom_host.cpp runs the same functions on
// the CPU).
//
// n is the index of the z a sample holds (z_1 = c).  N_n = x_n^2 + y_n^2 is the untruncated 2L-limb sum fsx::step forms for the
// escape test.  E is the first n at which z_n escapes; the sample's value is v = min(E - 1, cap).
//
// Atom period A.  The tracked states are z_1 .. z_v: those that passed the escape test with n <= cap (z_{cap+1} is tested before the
// cap test, and is NOT tracked).  A is the n in 1 .. v with the smallest N_n, ties to the EARLIEST n: a new minimum is strictly less,
// unsigned, over all 2L limbs.  v = 0 (c itself escapes) leaves A = 0.
//
// Cycle length lambda.  A sample the cycle check proves at index n equals its checkpoint, and under the rule of
// exact_cycle_math.hpp that checkpoint was taken at t = the largest power of two below n (z_1 for n = 2): lambda = n - t, a function
// of n alone.  0 for a sample that is not proved.
//
// A proved sample stops early and still has the A of the full cap: it holds z_n = z_t, so every state from n on is a copy of one of
// z_t .. z_{n-1}, which were tracked at an earlier index, and ties go to the earliest.  A therefore does not depend on the cycle
// check, and -- like lambda -- looks at n and N_n only, never at where a slice ends or at which slot a sample sits.
//
// The minimum lives in memory, per PIXEL: limb k of it is mn[k * stride + pix], k = 0 .. 2L - 1 (the device: 2L planes of W * H; the
// host: an array, stride 1, pix 0).  Where the planes are is itself in memory (AtomPlanes): the step loop carries one pointer, and the
// rare paths read the others through it.  What a lane keeps in registers is a 64-bit key of it, a monotone function of the 2L-limb value
// (a <= b gives key(a) <= key(b)): key less, take; key greater, not; key equal, read the minimum back and compare all limbs.  The key
// is (h, w[h], w[h-1] >> 6) in 6 + 32 + 26 bits, h the index of the highest limb that is not zero (0 when all are): it still tells
// values apart when the top limbs are zero, as they are near a nucleus, and it is made of selects on constant indices only.  The key
// of the minimum is kept in a plane of its own (keys[pix]) so that a slice reloads two registers, not 2L limbs.  `shift` drops the
// key's low bits (monotone still): 0 in the product; a test raises it, at most to kAtomMaxKeyShift where only h is left, to make the
// full compare run -- and answer "not less" -- often.
//
// Point runs (DESIGN.md 6.3 "Point runs"; fs_exact_eval_points, the S = true, P = true instantiations): the same rule on a list of
// runs with a length each in place of the cap, the period state per run, and the state z_len of every run that reaches its length
// left in end planes (point_end; the host loop is point_run).
#ifndef FS_EXACT_ATOM_MATH_HPP
#define FS_EXACT_ATOM_MATH_HPP

#include "exact_cycle_math.hpp"

namespace fsx {

constexpr uint32_t kAtomMaxKeyShift = 58; // the narrowest key: h alone

struct AtomPlanes {
    uint32_t *mn;     // 2L limb planes of `stride` pixels: the smallest norm so far (never initialised: n = 1 is always taken)
    uint64_t *keys;   // [stride]: the key of that minimum
    uint64_t *atom;   // [stride]: the index the minimum was taken at; zeroed by the caller
    uint64_t *cyclen; // [stride], with the cycle check: n - t of a proved sample; zeroed by the caller
    uint32_t stride;  // pixels
    uint32_t *end;    // point runs only (fs_exact_eval_points): 2L limb planes of `stride` runs, x then y: z_len; zeroed by the caller
};

// the shift that leaves the `bits` top bits of the key; 0 (and anything from 64 up) = all of them, below 6 = 6
inline uint32_t atom_key_shift(uint32_t bits)
{
    if (bits == 0 || bits >= 64)
        return 0;
    return bits < 64 - kAtomMaxKeyShift ? kAtomMaxKeyShift : 64 - bits;
}

// the key of the unsigned N-limb w
template <int N> FSX_HD uint64_t atom_key(const uint32_t (&w)[N], uint32_t shift)
{
    // From the top down, a limb's three selects finished before the next limb's condition is made: one condition is alive at a
    // time.  Left to itself the scheduler runs the chain of `top` ahead and keeps all N conditions -- a scalar register pair each --
    // for the selects of h and next (L = 18 and up then spill scalar registers).
    uint32_t h = N - 1, top = w[N - 1], next = w[N - 2];
    FSX_UNROLL
    for (int i = N - 2; i >= 0; i--) {
        const bool z = top == 0;
        h = z ? (uint32_t)i : h;
        top = z ? w[i] : top;
        next = z ? (i > 0 ? w[i > 0 ? i - 1 : 0] : 0u) : next;
        FSX_IN_ORDER();
    }
    return ((((uint64_t)h << 58) | ((uint64_t)top << 26) | (uint64_t)(next >> 6))) >> shift;
}

// the index the checkpoint of a sample proved at n (>= 2) was taken at, and the cycle length the proof shows
FSX_HD uint64_t cycle_checkpoint_index(uint64_t n) { return 1ull << (63 - __builtin_clzll(n - 1)); }
FSX_HD uint64_t cycle_length(uint64_t n) { return n - cycle_checkpoint_index(n); }

// The rare paths do not keep the sum the key was made of: they form xx + yy again, limb by limb as they need it, so that no path
// of the step loop holds a third 2L-limb number beside the two squares.  Each limb of xx is pinned on its way in (FSX_PIN: "may have
// changed") so that a compiler does not take the second sum for the first and keep that one -- or its 2L carries, a register pair
// of conditions each -- alive instead.
template <int L> FSX_HD uint32_t atom_sum_limb(const uint32_t (&xx)[2 * L], const uint32_t (&yy)[2 * L], int l, uint32_t &c)
{
    uint32_t a = xx[l];
    FSX_PIN(a);
    return addc(a, yy[l], c);
}

// the minimum becomes xx + yy, at index n
template <int L>
FSX_HD void atom_take(const uint32_t (&xx)[2 * L], const uint32_t (&yy)[2 * L], uint64_t n, uint64_t k, const AtomPlanes *planes,
                      uint32_t pix, uint64_t &kmin)
{
    uint32_t c = 0;
    FSX_PIN(planes); // (a vector register pair: what is read through it stays out of the scalar registers)
    FSX_PIN(pix);
    uint32_t *mn = planes->mn;
    uint64_t *keys = planes->keys, *atom = planes->atom;
    const uint32_t stride = planes->stride;
    FSX_UNROLL
    for (int l = 0; l < 2 * L; l++)
        mn[(size_t)l * stride + pix] = atom_sum_limb<L>(xx, yy, l, c);
    keys[pix] = k;
    atom[pix] = n;
    kmin = k;
}

// whether xx + yy is below the minimum in memory, unsigned, on all 2L limbs: the borrow out of (xx + yy) - minimum
template <int L>
FSX_HD bool atom_below(const uint32_t (&xx)[2 * L], const uint32_t (&yy)[2 * L], const AtomPlanes *planes, uint32_t pix)
{
    uint32_t c = 0, borrow = 0;
    FSX_PIN(planes); // (a vector register pair: what is read through it stays out of the scalar registers)
    FSX_PIN(pix);
    const uint32_t *mn = planes->mn;
    const uint32_t stride = planes->stride;
    FSX_UNROLL
    for (int l = 0; l < 2 * L; l++) {
        const uint32_t s = atom_sum_limb<L>(xx, yy, l, c), m = mn[(size_t)l * stride + pix];
        uint32_t d, e;
        const uint32_t b1 = __builtin_sub_overflow(s, m, &d) ? 1u : 0u;
        const uint32_t b2 = __builtin_sub_overflow(d, borrow, &e) ? 1u : 0u;
        borrow = b1 | b2;
    }
    return borrow != 0;
}

// The rule, for a state z_n that has passed the escape test, with squares xx, yy and norm w = xx + yy; tracked: n <= cap (as a
// condition of the two rare paths, not a branch around the whole rule: one nesting level less costs the kernel two scalar registers
// less).  True: it was a new minimum.  compares += 1 when the minimum was read back.
template <int L>
FSX_HD bool atom_track(const uint32_t (&xx)[2 * L], const uint32_t (&yy)[2 * L], const uint32_t (&w)[2 * L], uint64_t n, bool tracked,
                       const AtomPlanes *planes, uint32_t pix, uint64_t &kmin, uint32_t shift, uint32_t &compares)
{
    const uint64_t k = atom_key<2 * L>(w, shift);
    bool take = tracked && (n == 1 || k < kmin); // (n = 1 is taken unconditionally: the planes need no initial value)
    if (tracked && !take && k == kmin) {
        compares++;
        take = atom_below<L>(xx, yy, planes, pix);
    }
    if (take)
        atom_take<L>(xx, yy, n, k, planes, pix, kmin);
    return take;
}

// Point runs (fs_exact_eval_points; the S = true, P = true instantiations): run e has a length of its own, len[e], where a frame has its
// cap, and leaves the state it holds when it passes the escape test with n == len[e] -- z_len, before the step advances it -- in the
// end planes.  A run that escapes at or before len[e] leaves them as the caller zeroed them.
template <int L> FSX_HD void point_end(const uint32_t (&x)[L], const uint32_t (&y)[L], const AtomPlanes *planes, uint32_t e)
{
    FSX_PIN(planes); // (as atom_take: what is read through it stays out of the scalar registers)
    FSX_PIN(e);
    uint32_t *end = planes->end;
    const uint32_t stride = planes->stride;
    FSX_UNROLL
    for (int l = 0; l < L; l++) {
        end[(size_t)l * stride + e] = x[l];
        end[(size_t)(L + l) * stride + e] = y[l];
    }
}

struct AtomRun {
    uint32_t outcome;  // kCycleEscaped: value = E - 1; kCycleCapped, kCycleProved: value = cap
    uint64_t value;
    uint64_t atom;     // A
    uint64_t proof_n;  // the index the sample was proved at, 0: not proved
    uint64_t cyclen;   // lambda
    uint64_t steps;    // calls of step()
    uint64_t compares; // times the minimum was read back
};

// One sample from z_1 = c to its end: the loop of k_exact_slice<L, false, C, false, true> without the slices, check = C.  (Host
// loops and tests.)
template <int L>
FSX_HD AtomRun atom_run(const uint32_t (&cx)[L], const uint32_t (&cy)[L], const Params &P, uint64_t cap, bool check, uint32_t mx,
                        uint32_t my, uint32_t shift)
{
    uint32_t x[L], y[L], ck[2 * L], mn[2 * L], fx, fy, cycle_compares = 0, compares = 0;
    uint64_t n = 1, kmin = 0, key_plane = 0, atom = 0;
    const AtomPlanes planes{mn, &key_plane, &atom, nullptr, 1};
    AtomRun R{kCycleCapped, cap, 0, 0, 0, 0, 0};
    FSX_UNROLL
    for (int i = 0; i < L; i++)
        x[i] = cx[i], y[i] = cy[i];
    cycle_take<L>(x, y, ck, 1, 0, fx, fy);
    for (;;) {
        R.steps++;
        const bool escaped =
            step_with<L>(x, y, cx, cy, P, [&](const uint32_t (&xx)[2 * L], const uint32_t (&yy)[2 * L], const uint32_t (&w)[2 * L]) {
                atom_track<L>(xx, yy, w, n, n != cap + 1, &planes, 0, kmin, shift, compares);
            });
        if (escaped || n == cap + 1) {
            R.outcome = escaped ? kCycleEscaped : kCycleCapped;
            R.value = escaped ? n - 1 : cap;
            break;
        }
        n++;
        if (check && cycle_check<L>(x, y, n, ck, 1, 0, fx, fy, mx, my, cycle_compares)) {
            R.outcome = kCycleProved;
            R.proof_n = n, R.cyclen = cycle_length(n);
            break;
        }
    }
    R.atom = atom, R.compares = compares;
    return R;
}

struct PointRun {
    uint64_t value; // v = min(E - 1, len)
    uint64_t atom;  // A over z_1 .. z_v
    uint64_t steps; // calls of step()
};

// One point run from z_1 = c to its end: the loop of k_exact_slice<L, true, false, false, true> without the slices.  end: the 2L
// limbs of z_len, x then y, all zero when v < len.  (Host loops and tests.)
template <int L>
FSX_HD PointRun point_run(const uint32_t (&cx)[L], const uint32_t (&cy)[L], const Params &P, uint64_t len, uint32_t shift,
                          uint32_t (&end)[2 * L])
{
    uint32_t x[L], y[L], mn[2 * L], compares = 0;
    uint64_t n = 1, kmin = 0, key_plane = 0, atom = 0;
    const AtomPlanes planes{mn, &key_plane, &atom, nullptr, 1, end};
    const uint64_t cap1 = len + 1;
    PointRun R{len, 0, 0};
    FSX_UNROLL
    for (int i = 0; i < L; i++)
        x[i] = cx[i], y[i] = cy[i], end[i] = end[L + i] = 0;
    for (;;) {
        R.steps++;
        const bool escaped =
            step_with<L>(x, y, cx, cy, P, [&](const uint32_t (&xx)[2 * L], const uint32_t (&yy)[2 * L], const uint32_t (&w)[2 * L]) {
                if (n + 1 == cap1)
                    point_end<L>(x, y, &planes, 0);
                atom_track<L>(xx, yy, w, n, n != cap1, &planes, 0, kmin, shift, compares);
            });
        if (escaped || n == cap1) {
            R.value = escaped ? n - 1 : len;
            break;
        }
        n++;
    }
    R.atom = atom;
    return R;
}

} // namespace fsx

#endif
