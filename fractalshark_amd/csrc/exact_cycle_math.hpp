// exact_cycle_math.hpp -- the exact renderer's proof of non-escape by an exact repeat of the state (DESIGN.md 6.3 "Cycle check"),
// for the device (kernels_exact.hip, the C = true instantiations) and for the host (g++; tests/exact/exact_cycle_host.cpp runs the
// same functions on the CPU), and the park-and-resume rule of the continuation (fs_set_exact_keep; the K = true instantiations,
// tests/exact/exact_keep_host.cpp), at the end of the file.
//
// The arithmetic of exact_math.hpp is integer and nothing is rounded, so z_{k+1} is a function of z_k alone.  n is the index of the
// z a sample holds (z_1 = c).  If the z_n it holds equals, limb for limb, the z_m it held at an earlier m, then z_k = z_{k - (n - m)}
// for every k >= n: every later state is one of z_m .. z_{n-1}, and each of those has passed the escape test already (the sample
// would not have got to n otherwise).  The sample escapes at no cap, and its value is N.
//
// The rule.  Every sample carries a checkpoint (tx, ty) of 2L limbs, z_1 = c at n = 1.  After n++ the sample holds z_n:
//   * (x, y) == (tx, ty) on all 2L limbs: proved.
//   * otherwise, n a power of two: the checkpoint becomes (x, y).
// The escape test and the cap test come first (a sample that reaches n == cap + 1 finishes unproved); the rule looks at n only, so
// outcome and step count of a sample do not depend on where a slice ends.  A cycle of period p entered at step m is found at
// n = 2^j + p, 2^j the first power of two >= max(m, p): below 2 max(m, p) + p, with one checkpoint.
//
// The checkpoint lives in memory, not in registers: limb k of it is ck[k * stride + slot], k = 0 .. L - 1 for tx and L .. 2L - 1 for
// ty (the device: the sample's slot of the list's 2L limb planes; the host: an array, stride 1, slot 0).  What a lane keeps in registers is a fingerprint,
// the low limbs fx = tx[0] and fy = ty[0]; only when ((x[0] ^ fx) & mx) | ((y[0] ^ fy) & my) is zero does it read the checkpoint
// back.  The masks are the same for every sample of a call: all ones, unless a test narrows them to make the full compare run --
// and answer "not equal" -- often.
#ifndef FS_EXACT_CYCLE_MATH_HPP
#define FS_EXACT_CYCLE_MATH_HPP

#include <cstddef>

#include "exact_math.hpp"

// The addresses ck + k * stride + slot are invariants of the kernel's step loop, and a compiler that hoists them out of it keeps 2L
// 64-bit addresses -- 4L registers -- alive across the multiply (measured: 455 registers instead of 349 with 24 limbs; the address of
// limb 0 and of the proved byte alone are four).  They belong inside the rare paths.  An empty asm statement that may "change" the
// stride and the slot pins the arithmetic behind it; it holds no instruction.
#if defined(__HIP_DEVICE_COMPILE__)
#define FSX_PIN(v) asm volatile("" : "+v"(v))
#define FSX_IN_ORDER() __builtin_amdgcn_sched_barrier(0) // the instruction scheduler moves nothing across this line; no instruction
#else
#define FSX_PIN(v) ((void)0)
#define FSX_IN_ORDER() ((void)0)
#endif

namespace fsx {

// the fingerprint masks for `bits` low bits of the 64-bit number (y[0] : x[0]); 0 (and anything from 64 up) = all of them
inline void cycle_masks(uint32_t bits, uint32_t &mx, uint32_t &my)
{
    const uint64_t m = bits == 0 || bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
    mx = (uint32_t)m, my = (uint32_t)(m >> 32);
}

// the checkpoint becomes (x, y)
template <int L>
FSX_HD void cycle_take(const uint32_t (&x)[L], const uint32_t (&y)[L], uint32_t *ck, uint32_t stride, uint32_t slot, uint32_t &fx,
                       uint32_t &fy)
{
    FSX_PIN(stride);
    FSX_PIN(slot);
    FSX_UNROLL
    for (int l = 0; l < L; l++) {
        ck[(size_t)l * stride + slot] = x[l];
        ck[(size_t)(L + l) * stride + slot] = y[l];
    }
    fx = x[0], fy = y[0];
}

// The rule, for a sample that has just made its n++ and holds z_n = (x, y).  True: proved.  compares += 1 when the checkpoint was
// read back.
template <int L>
FSX_HD bool cycle_check(const uint32_t (&x)[L], const uint32_t (&y)[L], uint64_t n, uint32_t *ck, uint32_t stride, uint32_t slot,
                        uint32_t &fx, uint32_t &fy, uint32_t mx, uint32_t my, uint32_t &compares)
{
    if ((((x[0] ^ fx) & mx) | ((y[0] ^ fy) & my)) == 0) {
        compares++;
        uint32_t d = 0;
        FSX_PIN(stride);
        FSX_PIN(slot);
        FSX_UNROLL
        for (int l = 0; l < L; l++)
            d |= (x[l] ^ ck[(size_t)l * stride + slot]) | (y[l] ^ ck[(size_t)(L + l) * stride + slot]);
        if (d == 0)
            return true;
    }
    if ((n & (n - 1)) == 0)
        cycle_take<L>(x, y, ck, stride, slot, fx, fy);
    return false;
}

enum { kCycleEscaped = 0, kCycleCapped = 1, kCycleProved = 2 };
struct CycleRun {
    uint32_t outcome;  // kCycleEscaped: value = E - 1; kCycleCapped, kCycleProved: value = cap
    uint64_t value;
    uint64_t steps;    // calls of step()
    uint64_t compares; // times the checkpoint was read back
};

// ---- Keeping (fs_set_exact_keep, fs_render_exact_continue; DESIGN.md 6.3 "Continuation").
// step() tests z_n and replaces it in one call, so a sample that stops at n == cap + 1 holds z_{cap+2} with n still cap + 1: it has
// passed the escape test at cap + 1, and neither the n++ nor the rule at n = cap + 2 has happened -- a run with that cap never gets
// there, and its mask says "unproved".  That is the PARKED state: (x, y) = z_{cap+2}, n = cap + 1 and the checkpoint as it stands.
// Under a larger cap the same sample would have gone on with exactly those two things, so a resumed sample does them first
// (cycle_resume) and then enters the step loop as a running one does: the rule at cap + 2 is neither skipped nor run twice, nor run
// before anyone asked for a larger cap.  The step that made z_{cap+2} is not repeated: steps and read-backs of the two runs add up
// to those of one run with the larger cap.
// (The wave-per-sample kernel of kernels_exact_wide.hip tests before it steps and parks z_{cap+1} with n = cap + 1: it resumes as a
// running sample, and repeats the one escape test.)
template <int L, bool C>
FSX_HD bool cycle_resume(const uint32_t (&x)[L], const uint32_t (&y)[L], uint64_t &n, uint32_t *ck, uint32_t stride, uint32_t slot,
                         uint32_t &fx, uint32_t &fy, uint32_t mx, uint32_t my, uint32_t &compares)
{
    n++;
    if constexpr (C)
        return cycle_check<L>(x, y, n, ck, stride, slot, fx, fy, mx, my, compares);
    else
        return false;
}

// A sample between two runs: what a list holds of it (the fingerprint is read back from the checkpoint, as a slice does).
template <int L> struct CycleState {
    uint32_t x[L], y[L], ck[2 * L];
    uint64_t n;
};

// One sample from the state S to its end under `cap`: from z_1 = c (resume = false: S is set up here) or from a parked state
// (resume = true, cap above the one it was parked under).  A sample that ends capped leaves S parked.  check = false: the loop of
// the C = false kernels (no proof, no read-back).  (Host loops and tests.)
template <int L>
FSX_HD CycleRun cycle_run_from(CycleState<L> &S, bool resume, const uint32_t (&cx)[L], const uint32_t (&cy)[L], const Params &P,
                               uint64_t cap, bool check, uint32_t mx, uint32_t my)
{
    uint32_t fx, fy, compares = 0;
    CycleRun R{kCycleCapped, cap, 0, 0};
    if (!resume) {
        FSX_UNROLL
        for (int i = 0; i < L; i++)
            S.x[i] = cx[i], S.y[i] = cy[i];
        S.n = 1;
        cycle_take<L>(S.x, S.y, S.ck, 1, 0, fx, fy);
    } else {
        fx = S.ck[0], fy = S.ck[L];
        const bool proved = check ? cycle_resume<L, true>(S.x, S.y, S.n, S.ck, 1, 0, fx, fy, mx, my, compares)
                                  : cycle_resume<L, false>(S.x, S.y, S.n, S.ck, 1, 0, fx, fy, mx, my, compares);
        R.compares = compares;
        if (proved) {
            R.outcome = kCycleProved;
            return R;
        }
    }
    for (;;) {
        R.steps++;
        const bool escaped = step<L>(S.x, S.y, cx, cy, P);
        if (escaped || S.n == cap + 1) {
            R.outcome = escaped ? kCycleEscaped : kCycleCapped;
            R.value = escaped ? S.n - 1 : cap;
            break;
        }
        S.n++;
        if (check && cycle_check<L>(S.x, S.y, S.n, S.ck, 1, 0, fx, fy, mx, my, compares)) {
            R.outcome = kCycleProved;
            break;
        }
    }
    R.compares = compares;
    return R;
}

// One sample from z_1 = c to its end: the loop of k_exact_slice<L, S, true> without the slices.  (Host loops and tests.)
template <int L>
FSX_HD CycleRun cycle_run(const uint32_t (&cx)[L], const uint32_t (&cy)[L], const Params &P, uint64_t cap, uint32_t mx, uint32_t my)
{
    CycleState<L> S;
    return cycle_run_from<L>(S, false, cx, cy, P, cap, true, mx, my);
}

} // namespace fsx

#endif
