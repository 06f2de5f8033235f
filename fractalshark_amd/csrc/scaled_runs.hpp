// scaled_runs.hpp -- what the two HDRFloat<float> perturbation kernels share (round 6: moved out of kernels.hip when each kernel got
// a translation unit of its own -- kernels_lav2_hdr32.hip: k_lav2_hdr32_fast; kernels_perturb.hip: k_perturb_scalar): the step pieces
// of the scaled runs, the hand-scheduled untested loops (FS_FAST_LOOP_*), the run-length votes and the small key / scale helpers.
// One definition of each; the text is the one rounds 3-5 wrote (DESIGN_APPENDIX.md 4.2, 4.3).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdr_math.hpp"
#include "kernels.h"

namespace {

// max / min of two magnitudes as ONE instruction (source modifiers).  Written as fmaxf(fabsf(a), fabsf(b)) the compiler first
// canonicalises each operand (v_max_f32 |a|, |a| -- quieting a signalling NaN no arithmetic of this file can produce): three
// instructions instead of one at every run entry, run exit and tested step.  A quiet NaN in one operand returns the other, as
// fmaxf / fminf do.
static __device__ __forceinline__ float fs_max_abs(float a, float b)
{
    float r;
    asm("v_max_f32_e64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
static __device__ __forceinline__ float fs_min_abs(float a, float b)
{
    float r;
    asm("v_min_f32_e64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

} // namespace

namespace {
// A scaled run may start at entry e of the second companion array: a usable entry (bound not "never") or an exact zero.
__device__ __forceinline__ bool scaled_startable(const float4 e)
{
    return __float_as_int(e.z) != (int)0x80000000 || (e.x == 0.0f && e.y == 0.0f);
}
} // namespace

// ------------------------------------------------------------------------------------------------
// The scalar-cache path of the scaled runs (k_lav2_hdr32_fast and the perturbation-only float path of k_perturb_scalar):
// step pieces of the tested C++ block and the hand-scheduled untested loop.  Names used from the enclosing scope: sE2, dcs,
// Esh, imdc, wv, mxS, pwi, zS, off, zpb, lim8 (and the asm's outputs).
// PF of the loops (FS_FAST_LOOP_FL / _FD below): FS_PF_NONE, or FS_PF_NEXT_BODY = one dword of each 64-byte line of the NEXT body's entries (three:
// entries are 16-byte aligned only), requested right after this body's wait, so that the next body's loads hit the scalar
// cache -- for waves that run alone on their SIMD (C2's interior pixels), where the L2 round trip per body is not hidden.
#define FS_PF_NONE ""
#define FS_PF_NEXT_BODY                                                                                             \
    "s_load_dword %[pf], s[68:69], %[off] offset:0x80\n\t"                                                          \
    "s_load_dword %[pg], s[68:69], %[off] offset:0xc0\n\t"                                                          \
    "s_load_dword %[ph], s[68:69], %[off] offset:0xfc\n\t"
#define FS_STEP_ARITH(W_, Z_, NW_, T)                                                                               \
    const f2 s_##T = __builtin_elementwise_fma(W_, sE2, Z_);                                                        \
    const f2 pa_##T = W_.xx * s_##T;                                                                                \
    const f2 pb_##T = W_.yy * s_##T.yx;                                                                             \
    f2 p_##T;                                                                                                       \
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,0]" : "=v"(p_##T) : "v"(pa_##T), "v"(pb_##T));              \
    NW_ = p_##T + dcs;
#define FS_STEP_BOUND(NW_, T, V, EB)                                                                                \
    const float mx_##T = fs_max_abs(NW_.x, NW_.y);                           \
    V |= __builtin_amdgcn_ballot_w64(__float_as_int(mx_##T) + Esh > __float_as_int(EB));
// One scaled step with its acceptance tests, and the per-lane entry load of the runs whose lanes sit at different orbit
// positions: shared by k_lav2_hdr32_fast and the perturbation-only float path of k_perturb_scalar (one definition; round 4 had
// two identical copies).  Names from the enclosing scope as listed above, plus lane_off / zp for the load.
#define FS_SCALED_STEP(W_, Z_, NW_, NZ_, T, V, FULL, AFTER_ARITH, EX, EY, EB)                                       \
    const f2 s_##T = __builtin_elementwise_fma(W_, sE2, Z_);                                                        \
    const f2 pa_##T = W_.xx * s_##T;                                                                                \
    const f2 pb_##T = W_.yy * s_##T.yx;                                                                             \
    f2 p_##T;                                                                                                       \
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,0]" : "=v"(p_##T) : "v"(pa_##T), "v"(pb_##T));              \
    NW_ = p_##T + dcs;                                                                                              \
    float mx_##T = fs_max_abs(NW_.x, NW_.y);                                 \
    AFTER_ARITH;                                                                                                    \
    NZ_ = (f2){EX, EY};                                                                                             \
    V |= __builtin_amdgcn_ballot_w64(__float_as_int(mx_##T) + Esh > __float_as_int(EB));                            \
    if (FULL) {                                                                                                     \
        FS_STEP_FLOOR(NW_, V)                                                                                       \
        V |= __builtin_amdgcn_ballot_w64(!(mx_##T < FS_FL_HIGH_TRIP));                                              \
    } else {                                                                                                        \
        FS_STEP_FLOOR_FIRST(NW_, V)                                                                                 \
    }
#define FS_SCALED_LOAD(OFS, T, PIN)                                                                                 \
    asm volatile("global_load_dwordx3 %0, %2, %3 offset:" OFS : "=v"(ent_##T), "+v"(PIN) : "v"(lane_off), "s"(zp));
// The untested body.  Registers are named (the halves of a packed pair have no operand syntax): the state w in v[48:49];
// four state pairs v[48:55] in rotation (a trip = two steps: start state, first step, and the next trip's two while the
// verdict is pending); the entries in s[36:67].  A packed result cannot be read by the next instruction, so each trip's
// tests run in the wait states of the following trip's packed arithmetic, and its verdict arrives just before that trip's
// second step is written over the failed trip's start state: everything a failed trip needs is still in its registers,
// and what was computed past it is dropped.
// The loop runs inside the statement: bodies of eight steps while the block test passes and eight steps are left
// (status 0 on the way out: state in v[48:49], max|w| in v60, `off` = 16 bytes per step taken so far, s[64:65] / s67 =
// 2Z / block bound of the entry the state is at); status 1 / 2: the first / second trip of a block failed (start state /
// first step: v48 / v50, v52 / v54; `off` counts the steps before the trip, `eb` = the first arrival's bound).  The
// tests of a body's LAST trip run in the wait states of the next body's first two steps -- or on the way out.
#define FS_PK_F(W, Z) "v_pk_fma_f32 v[56:57], " W ", %[se], " Z "\n\t"
#define FS_PK_MA(W) "v_pk_mul_f32 v[58:59], " W ", v[56:57] op_sel_hi:[0,1]\n\t"
#define FS_PK_MB(W) "v_pk_mul_f32 v[56:57], " W ", v[56:57] op_sel:[1,1] op_sel_hi:[1,0]\n\t"
#define FS_PK_P "v_pk_add_f32 v[58:59], v[58:59], v[56:57] neg_lo:[0,1] neg_hi:[0,0]\n\t"
#define FS_PK_A(NW) "v_pk_add_f32 " NW ", v[58:59], %[dc]\n\t"
#define FS_R0 "v[48:49]"
#define FS_R1 "v[50:51]"
#define FS_R2 "v[52:53]"
#define FS_R3 "v[54:55]"
#define FS_T_X(A, B) "v_max_f32_e64 v60, |" A "|, |" B "|\n\t"

// ------------------------------------------------------------------------------------------------
// Round 4: the FLOOR form of the scaled runs' acceptance tests (k_lav2_hdr32_fast, and k_perturb_scalar's float path -- whose
// simpler version of the argument is given there).  Scale of a run: w = dz 2^-E with E = dz's exponent + 24, i.e. max|w| starts in [2^-24, 2^-23).
//
// Why a scaled step can differ from the reference's HDRFloatComplex step at all (Fractal.cpp:2646-2661: cur = 2Z + dz,
// p = dz cur, q = p + dc, Reduce): both carry out the same IEEE operations on the same real operands (the scale is a
// power of two), so the results agree bit for bit UNLESS
//   (u) an operation underflows -- its result is below 2^-126 in the units it is carried out in and loses bits -- in one
//       of the two arithmetics: the scaled one (units 2^E), or the reference's mantissa arithmetic (products in units of
//       2^(dz.e + cur.e), the aligned operand of an addition in the units of the larger one, Reduce's re-scaling by up to
//       2^-4).  Such an event injects an absolute error below 2^-126 in ITS units; in the run's units that is below
//       2^(-126 + 35): the exponent of a product's units is that of max|w| (kept below 29, see H) plus that of 2Z + dz
//       (< 5), and dc's units are at most 2^7 (start condition).  Two roundings lie between the event and a part of the
//       new state (p = a - b, q = p + dc), each amplifies the error by at most 2^26 relative to the result it rounds, so a
//       part of q that is wrong because of it is smaller than 2^(-91 + 29.2) < 2^-61;
//   (d) the reference DROPS the smaller operand of q = p + dc when the exponents are 120 or more apart
//       (HDRFloatComplex::plus_mutable) while the scaled step adds it: a part of q can differ only where the dropped
//       operand is within 2^26 of the kept one's part, and then that part of q is below 2^(28 + exponent of the kept
//       operand's units - 120) <= 2^-57 (dc dropped: units of p, < 2^35) or far below (p dropped: dc's units <= 2^7).
//       (cur = 2Z + dz: a dropped dz is more than 2^79 below either part of a usable orbit entry -- the companion's
//       "usable" test -- and changes no bit.)
// Hence: a new state whose TWO parts are both at least 2^-56 in magnitude (the floor, F) is the reference's state, bit for
// bit, provided the state it was stepped from was (induction) and had max|w| < 2^29 (H).  Every state is tested against
// the floor (one v_min / v_min3 per state, one compare per two states); H is tested where a block starts (max|w| < 2^14:
// a step multiplies max|w| by less than 25.2 and adds at most 2^7, so the block's other three states stay below 2^29).
// The form above tests every SECOND state and therefore needs a test relative to the state's size (part ratio 2^-40 and a
// 60-binade window: six vector instructions per two states instead of three).  Exact zero parts fail the floor (pixels on
// the axes go to the exponent-tracking loop, as before).
// Two forms (FS_FL_EVERY).  1 (the product) = every state against the floor 2^-56, as derived above: each state of a run is
// certified.  0 (only the FS_VERIFY_FLOOR build) = every SECOND state (a trip's second step) against the higher floor 2^-44 -- one
// v_min and one compare per two states instead of two and one: 49.0 instead of 51.5 ms on C3, the same frames on every
// test -- but its argument has a gap and it is NOT the default: the untested first state `a` of a trip can differ from the
// reference's in a part that is itself below 2^-60 (by less than 2^-86), and although that difference is 2^25 ulps below
// anything that matters in a second state b whose parts are at least 2^-44, it can still flip a rounding of b when one of
// b's intermediate sums happens to land within that distance of a rounding boundary (probability of the order of 2^-15
// per such trip).  tools/floor_check.py (FS_VERIFY_FLOOR build) counts the trips whose first state has a part below 2^-56
// while the second passes: about 1 in 10^4 wave-trips on C3's view -- rare, not absent.
#if defined(FS_VERIFY_FLOOR)
#define FS_FL_EVERY 0
#else
#define FS_FL_EVERY 1
#endif
// scale of a run: measured on C3 (every-state form): 20 / 24 / 28 -> 51.5 / 51.7 / 51.5 ms; second-state form 10 .. 28 in DESIGN.md
constexpr int kScaleShift = 24;
constexpr int kFloorExp = FS_FL_EVERY ? 56 : 44; // the floor 2^-kFloorExp (its margins: see above)
#define FS_FL_FLOOR __builtin_amdgcn_ldexpf(1.0f, -kFloorExp)
constexpr int kFloorBits = (127 - kFloorExp) << 23;
#define FS_FL_HIGH 0x1p14f   /* max|w| where a 4-step block starts */
#define FS_FL_HIGH_TRIP 0x1p24f /* the per-lane paths test H once per two-step trip: 25.2 * 2^24 + 2^7 < 2^29 */
#if defined(FS_VERIFY_FLOOR)
// VERIFICATION BUILD (tools/floor_check.py): the every-second-state form, plus a record of every trip whose FIRST state has a
// part below 2^-56 (the every-state floor) -- the only trips on which the two forms can differ at all.  The record is the
// sticky lane mask %[xa]; the caller counts the loop invocations that leave it non-zero.
#define FS_FL_N1(A, B) "v_min_f32_e64 v61, |" A "|, |" B "|\n\tv_cmp_gt_f32_e32 vcc, %[flr56], v61\n\ts_or_b64 %[xa], %[xa], vcc\n\t"
#define FS_FL_N2(A, B) "v_min_f32_e64 v61, |" A "|, |" B "|\n\t"
#else
#define FS_FL_N1(A, B) "v_min_f32_e64 v61, |" A "|, |" B "|\n\t"
#define FS_FL_N2(A, B) "v_min3_f32 v61, |" A "|, |" B "|, v61\n\t"
#endif
#define FS_FL_C "v_cmp_gt_f32_e32 vcc, %[flr], v61\n\t"   /* floor > the smallest part tested */
#define FS_FL_H "v_cmp_lt_f32_e32 vcc, 0x46800000, v60\n\t"   /* 2^14 < max|w| at a block's first state */
#define FS_STEP_FLOOR(NW_, V)                                                                                       \
    V |= __builtin_amdgcn_ballot_w64(!(fs_min_abs(NW_.x, NW_.y) >= FS_FL_FLOOR));
#if defined(FS_VERIFY_FLOOR)
#define FS_STEP_FLOOR_FIRST(NW_, V)                                                                                 \
    if (kStats && __builtin_amdgcn_ballot_w64(!(fs_min_abs(NW_.x, NW_.y) >= 0x1p-56f)) != 0ull) \
        c_blk_violation++;
#else
#define FS_STEP_FLOOR_FIRST(NW_, V) FS_STEP_FLOOR(NW_, V)
#endif
// The untested body, floor form (round 3's form of this statement tested every second state against a ratio and a window:
// six vector instructions per two states).  Registers, rotation of the four state pairs and exits as described above; a
// trip's two states (first step, second step) are tested together while the next trip's packed arithmetic is in flight,
// the verdict arrives before that trip's second step overwrites the failed trip's start state.  On entry the pending
// "previous trip" is (v[54:55], v[48:49]): the caller passes the entering state in both.
#define FS_FAST_LOOP_FL(PF)                                                                                           \
    asm volatile(                                                                                                   \
        ".Lfl_loop_%=:\n\t" /* eight steps left?  the first block's tests: max(max|w|, max|dc|) against .w (s67), H */ \
        "v_max_i32_e32 v62, v60, %[imdc]\n\t"                                                                       \
        "s_cmp_gt_u32 %[off], %[lim8]\n\t"                                                                          \
        "v_add_u32_e32 v62, v62, %[esh]\n\t"                                                                        \
        "s_cbranch_scc1 .Lfl_out_%=\n\t"                                                                            \
        "v_cmp_lt_i32_e64 %[m], s67, v62\n\t" FS_FL_H                                                               \
        "s_or_b64 %[m], %[m], vcc\n\t"                                                                              \
        "s_cbranch_scc1 .Lfl_out_%=\n\t" /* steps 1, 2 + the pending tests (previous body's last trip) */           \
        FS_PK_F(FS_R0, "s[64:65]") "s_mov_b32 %[eb], s62\n\t"                                                       \
        "s_load_dwordx16 s[36:51], s[68:69], %[off]\n\t"                                                            \
        "s_load_dwordx16 s[52:67], s[68:69], %[off] offset:0x40\n\t"                                                \
        FS_PK_MA(FS_R0) FS_FL_N1("v54", "v55") FS_PK_MB(FS_R0) FS_FL_N2("v48", "v49") FS_PK_P FS_FL_C FS_PK_A(FS_R1) \
        "s_waitcnt lgkmcnt(0)\n\t" PF                                                                               \
        FS_PK_F(FS_R1, "s[36:37]") FS_PK_MA(FS_R1) FS_PK_MB(FS_R1) FS_PK_P                                          \
        "s_cbranch_vccnz .Lfl_fp_%=\n\t" FS_PK_A(FS_R2) /* steps 3, 4 + the tests of trip 1 (v[50:51], v[52:53]) */ \
        FS_PK_F(FS_R2, "s[40:41]") FS_FL_N1("v50", "v51") FS_PK_MA(FS_R2) FS_PK_MB(FS_R2) FS_FL_N2("v52", "v53")    \
        FS_PK_P FS_FL_C FS_PK_A(FS_R3)                                                                              \
        FS_PK_F(FS_R3, "s[44:45]") FS_PK_MA(FS_R3) FS_PK_MB(FS_R3) FS_PK_P                                          \
        "s_cbranch_vccnz .Lfl_f1_%=\n\t" FS_PK_A(FS_R0) /* steps 5, 6 + the tests of trip 2 (v[54:55], v[48:49]) */ \
        FS_PK_F(FS_R0, "s[48:49]") FS_FL_N1("v54", "v55") FS_PK_MA(FS_R0) FS_PK_MB(FS_R0) FS_FL_N2("v48", "v49")    \
        FS_PK_P FS_FL_C FS_PK_A(FS_R1) FS_T_X("v48", "v49")                                                         \
        FS_PK_F(FS_R1, "s[52:53]") FS_PK_MA(FS_R1) FS_PK_MB(FS_R1) FS_PK_P                                          \
        "s_cbranch_vccnz .Lfl_f2_%=\n\t" /* the second block's tests: max(max|w4|, max|dc|) against entry 3's .w, H */ \
        "v_max_i32_e32 v62, v60, %[imdc]\n\t" FS_PK_A(FS_R2) "v_add_u32_e32 v62, v62, %[esh]\n\t"                   \
        /* steps 7, 8 + the tests of trip 3 (v[50:51], v[52:53]) */                                                 \
        FS_PK_F(FS_R2, "s[56:57]") "v_cmp_lt_i32_e64 %[m], s51, v62\n\t" FS_FL_H FS_PK_MA(FS_R2)                    \
        "s_or_b64 %[m], %[m], vcc\n\t" FS_PK_MB(FS_R2) FS_PK_P "s_cbranch_scc1 .Lfl_blk_%=\n\t" FS_PK_A(FS_R3)      \
        FS_FL_N1("v50", "v51")                                                                                      \
        FS_PK_F(FS_R3, "s[60:61]") FS_FL_N2("v52", "v53") FS_PK_MA(FS_R3) FS_PK_MB(FS_R3) FS_FL_C FS_PK_P           \
        "s_cbranch_vccnz .Lfl_f3_%=\n\t" FS_PK_A(FS_R0)                                                             \
        "s_add_u32 %[off], %[off], 0x80\n\t" /* max|w8| for the next block test; its floor test rides in the next body */ \
        FS_T_X("v48", "v49") "s_branch .Lfl_loop_%=\n"                                                              \
        ".Lfl_out_%=:\n\t" /* the block here needs its bound tests, or fewer than 8 steps are left: the pending tests */ \
        "s_mov_b32 %[eb], s62\n\t" FS_FL_N1("v54", "v55") FS_FL_N2("v48", "v49") FS_FL_C                            \
        "s_cbranch_vccnz .Lfl_fp_%=\n\t"                                                                            \
        "s_mov_b32 %[st], 0\n\t"                                                                                    \
        "s_branch .Lfl_end_%=\n"                                                                                    \
        ".Lfl_blk_%=:\n\t" /* the same after the first block (no verdict is pending there) */                       \
        "s_mov_b32 %[st], 0\n\t"                                                                                    \
        "s_mov_b64 s[64:65], s[48:49]\n\t"                                                                          \
        "s_mov_b32 s67, s51\n\t"                                                                                    \
        "s_add_u32 %[off], %[off], 0x40\n\t"                                                                        \
        "s_branch .Lfl_end_%=\n"                                                                                    \
        ".Lfl_fp_%=:\n\t" /* the previous body's last trip: start state v[52:53], first step v[54:55] */            \
        "s_mov_b32 %[st], 2\n\t"                                                                                    \
        "s_sub_u32 %[off], %[off], 0x20\n\t"                                                                        \
        "s_branch .Lfl_end_%=\n"                                                                                    \
        ".Lfl_f1_%=:\n\t"                                                                                           \
        "s_mov_b32 %[st], 1\n\t"                                                                                    \
        "s_mov_b32 %[eb], s38\n\t"                                                                                  \
        "s_branch .Lfl_end_%=\n"                                                                                    \
        ".Lfl_f2_%=:\n\t"                                                                                           \
        "s_mov_b32 %[st], 2\n\t"                                                                                    \
        "s_mov_b32 %[eb], s46\n\t"                                                                                  \
        "s_add_u32 %[off], %[off], 0x20\n\t"                                                                        \
        "s_branch .Lfl_end_%=\n"                                                                                    \
        ".Lfl_f3_%=:\n\t"                                                                                           \
        "s_mov_b32 %[st], 1\n\t"                                                                                    \
        "s_mov_b32 %[eb], s54\n\t"                                                                                  \
        "s_add_u32 %[off], %[off], 0x40\n"                                                                          \
        ".Lfl_end_%=:\n\t"                                                                                          \
        "s_waitcnt lgkmcnt(0)" /* (a failed pending trip leaves after the loads: nothing stays in flight) */        \
        : "+{v[48:49]}"(wv), "={v[50:51]}"(r1), "={v[52:53]}"(r2), "+{v[54:55]}"(r3), "={v[56:57]}"(ts_),           \
          "={v[58:59]}"(ta_), "+{v60}"(mxS), "={v61}"(tn_), "={v62}"(tl_), [m] "=&s"(msk_), [st] "=&s"(st),         \
          [eb] "=&s"(ebo), "+{s67}"(pwi), "+{s[64:65]}"(zS), [off] "+s"(off), [pf] "=&s"(pf_), [pg] "=&s"(pg_),     \
          [ph] "=&s"(ph_), [xa] "+s"(xacc_)                                                                         \
        : [se] "v"(sE2), [dc] "v"(dcs), [esh] "v"(Esh), [imdc] "v"(imdc), [lim8] "s"(lim8), "{s[68:69]}"(zpb),      \
          [flr] "s"(kFloorBits), [flr56] "s"((127 - 56) << 23)                                                      \
        : "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50",  \
          "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s66", "vcc",  \
          "scc")

// The untested body with the floor verdict DEFERRED (every-state form only): one v_min3 per state accumulates the smallest
// part of every state the invocation passes through (v61, +inf on entry: the entering state has been certified by whoever
// made it), no compare and no branch per trip; the verdict is taken once, on the way out -- status 3 = some state fell below
// the floor: the caller discards the whole run attempt (nothing has been committed) and repeats it with FS_FAST_LOOP_FL,
// whose per-trip verdicts stop at the failing trip.  A state below the floor is rare (about 1 in 10^4 wave-trips on C3), the
// repeat costs next to nothing, and each state of an accepted invocation has been tested exactly as in the per-trip form --
// every-state rigour at the price of the every-second-state form.  H and the block bounds are tested where a block starts,
// as in FS_FAST_LOOP_FL (they guard the steps that follow, so they cannot be deferred).
#define FS_FL_ACC(A, B) "v_min3_f32 v61, |" A "|, |" B "|, v61\n\t"
#define FS_BT_DC_MAX "v_max_i32_e32 v62, v60, %[imdc]\n\t"
#define FS_BT_DC_ADD "v_add_u32_e32 v62, v62, %[esh]\n\t"

// The untested body with the deferred verdict and the block test on WAVE-UNIFORM thresholds (round 5): the kernel issues one
// vector instruction per SIMD every four cycles and nothing else, and round 4's per-lane block test was five of them per four
// steps (max|w|, max with max|dc|, + the lane's scale, the compare, H's compare).  Both sides of it that are not the state are
// made scalar, each in the safe direction:
//   max|dc| 2^E is the pixel's true max|dc|, a constant: its largest value over the wave (`sdc`, made once per tile) is compared
//     with the block bound on the scalar unit;
//   bits(max|w|) + Esh <= bound holds in every lane when bits(max|w|) <= bound - (the LARGEST Esh of the running lanes: `eshm`,
//     made once per run by a few votes);  H is bits(max|w|) <= bits(2^14);
// so a block's test is  bits(max|w|) <= T,  T = min(bound - eshm, bits(2^14)), or -1 ("never") when sdc > bound -- which the
// "never" bound, the most negative integer, always is: five scalar instructions, then max|w| and ONE compare on the vector unit.
// (For a usable bound, >= 0, the difference can only overflow upwards, and an overflow means T = H; what the first three
// instructions make of the "never" bound is overwritten.  The first form of this macro replaced that bound by -2^30 and
// subtracted: positive again under a scale shift below -2^30, i.e. for |dz| < 2^-152 -- tools/block_bound_check.py counted 24 150
// such blocks among 3.6e9 on the deep views 11, 14 and 19, none on View 5.)  A wave whose lanes' scales are k binades
// apart tests its lower lanes against a bound 2^k tighter than theirs: such a block takes the tested path, nothing else changes.
// (FS_BT_TH: the same five instructions for any cap HB on max|w| -- H = 2^14 where a four-step block starts, FS_BT_T; Hz = 2^-5
// where an eight-step body of the form without the dz add starts, FS_BT_T2 below.)
#define FS_BT_THC(BW, BC, HB)                                                                                       \
    "s_sub_i32 %[t], " BW ", %[eshm]\n\t"                                                                           \
    "s_cselect_b32 %[t], " HB ", %[t]\n\t"                                                                          \
    "s_min_i32 %[t], %[t], " HB "\n\t"                                                                              \
    "s_cmp_gt_i32 %[sdc], " BC "\n\t"                                                                               \
    "s_cselect_b32 %[t], -1, %[t]\n\t"
#define FS_BT_TH(BW, HB) FS_BT_THC(BW, BW, HB)
#define FS_BT_T(BW) FS_BT_TH(BW, "0x46800000")
#define FS_BT_V "v_cmp_lt_i32_e32 vcc, %[t], v60\n\t"
// ---- ADD-FREE form of the body (ND, "no dc"): the step without its last instruction.
// A step ends with q = p + dc 2^-E (FS_PK_A).  On a deep view that sum is p, bit for bit: View 5's |dc| is near 2^-146 while
// the |dz| this loop sees is tens of binades above it.  The ND form writes p straight into the next state pair (FS_PK_PN) and
// issues four packed instructions per step instead of five.  When that is exact:
//   fl(p + d) == p  whenever  |d| <= 2^-26 |p|:  d is then strictly below half an ulp of p, also where |p| is a power of two and
//   the ulp below it is half the one above (2^-26 |p| = a quarter of the smaller ulp 2^-24 |p|), so round-to-nearest returns p.
//   Per lane and run  F_run = max(2^-56, 2^26 max(|dcs.x|, |dcs.y|)),  dcs = dc 2^-E, the run's scaled dc (|dcs| < 2^7 by the
//   start condition, so F_run is finite; a run whose F_run is not -- a NaN part -- is not eligible).
//   In an ND run every state IS its p, so the floor accumulator v61 -- the smallest part of every state of the invocation -- already
//   holds what has to be compared:  v61 >= F_run  certifies, for every step at once and in both parts, |dcs part| <= 2^-26 |p part|,
//   i.e. that the full form's add would have returned p.  Induction over the invocation: the entering state is the full form's
//   (whoever made it used the full form, or an ND invocation that passed this verdict), each ND state equals the full form's
//   state bit for bit, hence so does the next.  Because the states are the same bits, everything argued above for the full
//   form holds unchanged: the floor (F_run >= 2^-56 subsumes it), H, the bound tests, the block test on sdc / eshm.
//   The verdict is taken on the way out of the statement (status 5 = failed) against F_run, which is made there from dcs (three
//   instructions per invocation) instead of being held in a register across the loop.  A failed verdict commits nothing, as
//   status 3 commits nothing: the caller repeats the run from its parked start state in the full form.  (A state below the
//   floor 2^-56 itself is reported as status 3, as the full form reports it: that is the floor's business, not dc's, the run
//   is repeated with the per-trip verdicts as before and no back-off follows.)
//   Which form runs is decided once per run by the caller (%[nd], wave-uniform): every running lane's entering
//   min(|w0.x|, |w0.y|) >= F_run, otherwise the run takes the full form without trying; after refused entries or failed
//   verdicts in a row the wave sits out 0, 1, 2, 4, .. runs, up to kNdBackoffEntry / kNdBackoffVerdict (see there), so a shallow
//   view, whose dc is never negligible, pays one vote every kNdBackoffEntry runs.  The tested C++ blocks, the per-lane path, the hot runs, the careful
//   step and FS_FAST_LOOP_FL always add dc.
// Both forms live in ONE statement (a statement exit plus a run entry costs about 75 vector instructions); the full form is
// the text of round 5, instruction for instruction.  STEP_PRE / STEP_POST are the end of a step: FS_PK_P then FS_PK_A (full),
// nothing then FS_PK_PN (ND) -- split in two because the second block's branch sits between them.
#define FS_PK_PN(NW) "v_pk_add_f32 " NW ", v[58:59], v[56:57] neg_lo:[0,1] neg_hi:[0,0]\n\t"
// ---- The form without the dz add either (NDZ): an ND step without its FIRST instruction.
// A step starts with s = fma(w, 2^E, 2Z) (FS_PK_F).  Where |dz| is tens of binades below |Z| -- most steps of a deep view -- that
// is 2Z, bit for bit, and the NDZ step multiplies w by the entry's scalar register pair directly: three packed instructions
// (FS_PK_ZA, FS_PK_ZB, FS_PK_PN) and the state's v_min3.  Unlike ND's, its condition is known BEFORE the steps, from the orbit
// alone, so it is a threshold test where a body starts and needs no verdict afterwards.
//   The bounds.  k_make_quiet_orbit stores per orbit entry j the two NDZ BODY bounds (third companion, `znz`, a float2 per entry): on
//   D = max|dz| and on C = max|dc| in true scale at entry j.  With lo_k = min(|2Z_k.re|, |2Z_k.im|), the growth an NDZ step really has,
//   s_k = (|2Z_k.re| + |2Z_k.im|)(1 + 2^-10) (2Z as this loop reads it), A_0 = 1, B_0 = 0, A_(m+1) = s_(j+m) A_m, B_(m+1) = s_(j+m) B_m + 1:
//     .x = min over m = 0 .. 7 of 2^-27 lo_(j+m) / A_m,   .y = min over m = 1 .. 7 of 2^-27 lo_(j+m) / B_m,
//     each also within half of scaled_bound(Z_(j+8)) over A_8 / B_8 -- the eighth arrival's own bound test --, times (1 - 2^-10);
//   both "never" when one of the entries j + 1 .. j + 8 has no usable bound or an entry j .. j + 7 has M >= 5.6 (scaled_block_bound(j)
//   or (j + 4) is "never"), when a part of some 2Z is zero or below 2^-100, when a result is below 2^-120 (the integer compare of bit
//   patterns below needs a normal number) or when j + 8 is past the orbit.  (Round 8 kept one bound on max(D, C) and divided by
//   scaled_block_bound's g_k = 4 M_k + 3.8, valid for any G <= 1.4: 2^18 .. 2^21 over seven typical steps, so a body was refused until dz
//   was 2^-40 and more below Z where 2^-26 is what exactness needs.  One bound with the growth s + 1 came first and its counting launch
//   said what dc's own term would add: ndz_body_bound in kernels_orbit_prep.hip has the figures.)
//   1. Induction.  fl(a + d) == a whenever |d| <= 2^-26 |a| (argued for ND above).  The fma rounds once, and the product w 2^E is
//      exact inside it (a power of two; it IS dz in true scale, which need not be representable on its own).  Hypothesis at step m
//      (m = 0: D <= .x <= 2^-27 lo_j):  max|dz_m| <= A_m D + B_m C <= 2^-26 lo_(j+m), each half within 2^-27 lo_(j+m).
//        => |dz part| <= 2^-26 |2Z part| in BOTH parts of every lane: s == 2Z, and the NDZ state is the ND state bit for bit -- which
//           is the full form's once the ND verdict passes, as before: NDZ states are ND states, counted, floored (v61) and
//           certified against F_run like them;
//        => dz_(m+1) = dz_m 2Z + dc with |re| <= |dz.re| |2Z.re| + |dz.im| |2Z.im| + |dc.re| <= (|2Z.re| + |2Z.im|) max|dz_m| + C, the
//           imaginary part alike; the products and sums round 2^-24 relative each, 1 + 2^-10 covers them:
//           max|dz_(m+1)| <= s (A_m D + B_m C) + C = A_(m+1) D + B_(m+1) C;
//        => the hypothesis at m + 1 by the terms m + 1 of .x and .y (m + 1 <= 7);
//        => arrival m + 1 passes its bound test: 2^-26 lo <= 2^-25 zmax <= 2^-2 zmax = scaled_bound of a usable entry (lo <= 2 zmax);
//           the eighth arrival by the halves of scaled_bound(Z_(j+8)).
//   2. The wave-uniform threshold.  D <= .x is tested as the block test is, and is safe for every lane for the same reasons:
//      bits(max|w|) <= .x - eshm implies bits(max|w|) + Esh <= .x in each lane because eshm is the LARGEST Esh of the running lanes,
//      and sdc, the wave's largest max|dc|, stands for the lanes' max|dc| against .y.  T2 = min(.x - eshm, bits(Hz)), -1 when
//      sdc > .y: FS_BT_T's five instructions with another cap and the second bound in the compare (FS_BT_THC).
//      T2 against T.  Round 8's bound was within scaled_block_bound(j) and (j + 4), so a body that passed T2 would have passed the block
//      tests.  These bounds are not, and need not be: FS_NDZ_TAIL and .Lfz_entry compute T afresh when T2 refuses; the NDZ body has no
//      test inside, 1. vouches for its eight arrivals directly; where the NDZ loop leaves through .Lfn_out the caller takes a
//      TESTED block (or ends the run), which tests every arrival itself; the counting build's c_blk_free counts the blocks the
//      statement took, tested or vouched for.  What did lean on it is the counting build's REPLAY: the full form has to reach
//      the add-free invocation's end to be compared with it, see there (block tests waived up to the last body, then as usual).
//      Hz = 2^-5.  H asks for max|w| < 2^29 at every state a step leaves from; a body has no test inside, so its entering state
//      has to vouch for the seven states after it.  In true scale G grows by at most g <= (4 * 5.6 + 3.8)(1 + 2^-10) < 26.23 a
//      step (h <= (22.4 + 1)(1 + 2^-10) is below that), dc included, i.e. max(max|w|, max|dcs|) grows by that in the run's scale,
//      and 26.23^7 < 2^33: the seven states stay
//      below 2^33 max(2^-5, max|dcs|) = 2^28 -- an ND run's max|dcs| is below 2^-49 (its entry vote: 2^26 max|dcs| <= a part of a
//      state whose max is below 2^-23).  The eighth arrival (< 2^33) is the next decision's business: it fails Hz and H alike and
//      the statement ends in front of it.  A run starts with max|w| < 2^-23 and View 5 gains 0.007 binades a step: Hz never binds.
//   3. No test inside the body.  The full and ND bodies test w4 against the second block's T half way; the NDZ body needs none:
//      1. covers all eight arrivals from the state the body starts with.
//   The decision is taken where a body ends, for the next body, in the ND and the NDZ loop alike: max|w| against T2 first; when no
//   lane exceeds it the next body is NDZ, otherwise today's compare against T follows and the ND loop goes on or ends.  An NDZ body
//   is 24 packed + 8 v_min3 + 1 v_max + 1 v_cmp (4.25 per step, ND: 5.5); an ND body after a refused T2 pays one compare more.
//   The bounds of the next body's entry (s[72:73]) are loaded with the body's entries, from s[70:71] + off / 2; the statement reads the
//   bound of the entry it starts at itself (ND side only), so nothing about NDZ is live outside it.  The full form, the tested
//   blocks, the per-lane path, FS_FAST_LOOP_FL, the hot runs and the careful step never take it.
#define FS_NDZ_HZ "0x3d000000" /* bits(2^-5) */
#define FS_BT_T2(BD, BC) FS_BT_THC(BD, BC, FS_NDZ_HZ) /* max|w| against the D bound, max|dc| against the C bound */
#define FS_PK_ZA(W, Z) "v_pk_mul_f32 v[58:59], " W ", " Z " op_sel_hi:[0,1]\n\t"
#define FS_PK_ZB(W, Z) "v_pk_mul_f32 v[56:57], " W ", " Z " op_sel:[1,1] op_sel_hi:[1,0]\n\t"
#define FS_NDZ_STEP(W, WA, WB, Z, NW) FS_PK_ZA(W, Z) FS_FL_ACC(WA, WB) FS_PK_ZB(W, Z) FS_PK_PN(NW)
// the next body's NDZ bound, requested with the body's entries (%[t] is free between a body's verdict and its next FS_BT_T)
#define FS_NDZ_LOAD                                                                                                 \
    "s_lshr_b32 %[t], %[off], 1\n\t"                                                                                \
    "s_load_dwordx2 s[72:73], s[70:71], %[t] offset:0x40\n\t"
// where a body ends: today's (full form) / the NDZ decision first (ND and NDZ loops)
#define FS_FDU_TAIL(L) FS_BT_T("s67") FS_T_X("v48", "v49") FS_FL_ACC("v48", "v49") FS_BT_V "s_branch .L" L "_loop_%=\n"
#define FS_NDZ_TAIL                                                                                                 \
    FS_BT_T2("s72", "s73") FS_T_X("v48", "v49") FS_FL_ACC("v48", "v49") FS_BT_V                                            \
    "s_cbranch_vccz .Lfz_loop_%=\n\t" FS_BT_T("s67") FS_BT_V "s_branch .Lfn_loop_%=\n"
// the NDZ loop (CNT: the counting build's step counter, or nothing).  On the way out (fewer than eight steps left) it joins the
// ND loop's exit: the state in v[48:49], max|w| in v60, s[64:65] / s67 of the entry the state is at, as the ND loop leaves them.
#define FS_NDZ_LOOP(PF, CNT)                                                                                        \
        ".Lfz_loop_%=:\n\t"                                                                                         \
        "s_cmp_gt_u32 %[off], %[lim8]\n\t"                                                                          \
        "s_cbranch_scc1 .Lfn_out_%=\n\t"                                                                            \
        FS_PK_ZA(FS_R0, "s[64:65]") FS_PK_ZB(FS_R0, "s[64:65]")                                                     \
        "s_load_dwordx16 s[36:51], s[68:69], %[off]\n\t"                                                            \
        "s_load_dwordx16 s[52:67], s[68:69], %[off] offset:0x40\n\t"                                                \
        FS_NDZ_LOAD FS_PK_PN(FS_R1) CNT                                                                             \
        "s_waitcnt lgkmcnt(0)\n\t" PF                                                                               \
        FS_NDZ_STEP(FS_R1, "v50", "v51", "s[36:37]", FS_R2) FS_NDZ_STEP(FS_R2, "v52", "v53", "s[40:41]", FS_R3)     \
        FS_NDZ_STEP(FS_R3, "v54", "v55", "s[44:45]", FS_R0) FS_NDZ_STEP(FS_R0, "v48", "v49", "s[48:49]", FS_R1)     \
        FS_NDZ_STEP(FS_R1, "v50", "v51", "s[52:53]", FS_R2) FS_NDZ_STEP(FS_R2, "v52", "v53", "s[56:57]", FS_R3)     \
        FS_NDZ_STEP(FS_R3, "v54", "v55", "s[60:61]", FS_R0)                                                         \
        "s_add_u32 %[off], %[off], 0x80\n\t" FS_NDZ_TAIL
#define FS_FDU_LOOP(L, PF, PRE, POST, XLOAD, TAIL)                                                                  \
        ".L" L "_loop_%=:\n\t" /* eight steps left?  the first block's verdict (taken where max|w| was made) */      \
        "s_cmp_gt_u32 %[off], %[lim8]\n\t"                                                                          \
        "s_cbranch_scc1 .L" L "_out_%=\n\t"                                                                         \
        "s_cbranch_vccnz .L" L "_out_%=\n\t" /* steps 1 .. 4 */                                                     \
        FS_PK_F(FS_R0, "s[64:65]")                                                                                  \
        "s_load_dwordx16 s[36:51], s[68:69], %[off]\n\t"                                                            \
        "s_load_dwordx16 s[52:67], s[68:69], %[off] offset:0x40\n\t" XLOAD                                          \
        FS_PK_MA(FS_R0) FS_PK_MB(FS_R0) PRE POST(FS_R1)                                                             \
        "s_waitcnt lgkmcnt(0)\n\t" PF FS_BT_T("s51")                                                                \
        FS_PK_F(FS_R1, "s[36:37]") FS_FL_ACC("v50", "v51") FS_PK_MA(FS_R1) FS_PK_MB(FS_R1) PRE POST(FS_R2)          \
        FS_PK_F(FS_R2, "s[40:41]") FS_FL_ACC("v52", "v53") FS_PK_MA(FS_R2) FS_PK_MB(FS_R2) PRE POST(FS_R3)          \
        FS_PK_F(FS_R3, "s[44:45]") FS_FL_ACC("v54", "v55") FS_PK_MA(FS_R3) FS_PK_MB(FS_R3) PRE POST(FS_R0)          \
        /* step 5 + w4's floor part and max; the second block's verdict in step 6, before anything of block 2 is counted */ \
        FS_PK_F(FS_R0, "s[48:49]") FS_FL_ACC("v48", "v49") FS_PK_MA(FS_R0) FS_T_X("v48", "v49") FS_PK_MB(FS_R0)     \
        PRE POST(FS_R1)                                                                                             \
        FS_PK_F(FS_R1, "s[52:53]") FS_BT_V FS_PK_MA(FS_R1) FS_PK_MB(FS_R1) PRE                                      \
        "s_cbranch_vccnz .L" L "_blk_%=\n\t" POST(FS_R2)                                                            \
        FS_PK_F(FS_R2, "s[56:57]") FS_FL_ACC("v50", "v51") FS_PK_MA(FS_R2) FS_FL_ACC("v52", "v53") FS_PK_MB(FS_R2)  \
        PRE POST(FS_R3)                                                                                             \
        FS_PK_F(FS_R3, "s[60:61]") FS_FL_ACC("v54", "v55") FS_PK_MA(FS_R3) FS_PK_MB(FS_R3) PRE POST(FS_R0)          \
        "s_add_u32 %[off], %[off], 0x80\n\t" TAIL                                                                   \
        ".L" L "_blk_%=:\n\t" /* the second block needs its bound tests (or H): the state is w4 in v[48:49] */       \
        "s_mov_b64 s[64:65], s[48:49]\n\t"                                                                          \
        "s_mov_b32 s67, s51\n\t"                                                                                    \
        "s_add_u32 %[off], %[off], 0x40\n"                                                                          \
        ".L" L "_out_%=:\n\t"
#define FS_NDZ_COUNT "s_add_u32 %[nz], %[nz], 8\n\t" /* (counting build) wave-steps taken in NDZ bodies */
#define FS_FAST_LOOP_FDU(PF, CNT)                                                                                   \
    asm volatile(                                                                                                   \
        "v_mov_b32_e32 v61, 0x7f800000\n\t" FS_BT_T("s67") FS_BT_V                                                  \
        "s_cmp_lg_u32 %[nd], 0\n\t"                                                                                 \
        "s_cbranch_scc1 .Lfz_entry_%=\n"                                                                            \
        FS_FDU_LOOP("fu", PF, FS_PK_P, FS_PK_A, "", FS_FDU_TAIL("fu")) /* the verdict over every state of this invocation */ \
        "s_mov_b32 %[st], 0\n\t" FS_FL_C                                                                            \
        "s_cbranch_vccz .Lfu_end_%=\n\t"                                                                            \
        "s_mov_b32 %[st], 3\n\t"                                                                                    \
        "s_branch .Lfu_end_%=\n"                                                                                    \
        ".Lfz_entry_%=:\n\t" /* ND side: the NDZ bound of the entry the state is at, then the decision as where a body ends */ \
        "s_lshr_b32 %[t], %[off], 1\n\t"                                                                            \
        "s_load_dwordx2 s[72:73], s[70:71], %[t]\n\t"                                                               \
        "s_waitcnt lgkmcnt(0)\n\t" FS_BT_T2("s72", "s73") FS_BT_V                                                          \
        "s_cbranch_vccz .Lfz_loop_%=\n\t" FS_BT_T("s67") FS_BT_V                                                    \
        "s_branch .Lfn_loop_%=\n"                                                                                   \
        FS_NDZ_LOOP(PF, CNT)                                                                                        \
        FS_FDU_LOOP("fn", PF, "", FS_PK_PN, FS_NDZ_LOAD, FS_NDZ_TAIL) /* the ND verdict: F_run > the smallest part of any state */ \
        "v_max_f32_e64 v62, |%[dcx]|, |%[dcy]|\n\t"                                                                 \
        "s_mov_b32 %[st], 0\n\t"                                                                                    \
        "v_ldexp_f32 v62, v62, 26\n\t"                                                                              \
        "v_max_f32_e32 v62, %[flr], v62\n\t"                                                                        \
        "v_cmp_gt_f32_e32 vcc, v62, v61\n\t"                                                                        \
        "s_cbranch_vccz .Lfu_end_%=\n\t" /* failed: below the floor itself (3, as in the full form), or only below F_run (5) */ \
        "s_mov_b32 %[st], 5\n\t" FS_FL_C                                                                            \
        "s_cbranch_vccz .Lfu_end_%=\n\t"                                                                            \
        "s_mov_b32 %[st], 3\n"                                                                                      \
        ".Lfu_end_%=:\n\t"                                                                                        \
        "s_waitcnt lgkmcnt(0)"                                                                                      \
        : "+{v[48:49]}"(wv), "={v[50:51]}"(r1), "={v[52:53]}"(r2), "={v[54:55]}"(r3), "={v[56:57]}"(ts_),           \
          "={v[58:59]}"(ta_), "+{v60}"(mxS), "={v61}"(tn_), "={v62}"(tl_), [t] "=&s"(bt_t_), [st] "=&s"(st),        \
          "+{s67}"(pwi), "+{s[64:65]}"(zS), [off] "+s"(off), [pf] "=&s"(pf_), [pg] "=&s"(pg_), [ph] "=&s"(ph_),     \
          [nz] "+s"(nz_)                                                                                            \
        : [se] "v"(sE2), [dc] "v"(dcs), [dcx] "v"(dcs.x), [dcy] "v"(dcs.y), [eshm] "s"(Esh_cap),                    \
          [sdc] "s"(sdc_bits), [lim8] "s"(lim8), [nd] "s"(nd_sel), "{s[68:69]}"(zpb), "{s[70:71]}"(znp),            \
          [flr] "s"(kFloorBits)                                                                                     \
        : "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50",  \
          "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s66", "s72",  \
          "s73", "vcc", "scc")
// Runs for which a wave does not ask for the ND form again after an entry vote that refused it / after a failed verdict (which
// costs the run's steps a second time): a wave-uniform penalty that follows what happened.  It starts at 0 -- the wave asks again
// at the very next run: a verdict fails where the orbit passes a near-zero entry and dz 2Z drops to dc's size, the repeated run
// has passed that place and the next one is usually eligible again --, each further refusal or failure in a row doubles it
// (1, 2, 4, ..), capped at kNdBackoffEntry runs after a refused vote and kNdBackoffVerdict after a failed verdict, and an add-free
// invocation that takes steps and passes its verdict resets it.  A shallow view, whose dc is never negligible, still converges to
// one vote every kNdBackoffEntry runs, and a failed verdict cannot repeat at full cost run after run.  (Round 7's constants sat
// out 8 / 32 runs after the FIRST refusal / failure.)  Which form a run takes changes no result.
constexpr uint32_t kNdBackoffEntry = 8;
constexpr uint32_t kNdBackoffVerdict = 32;
// The back-off state after a refusal: runs to sit out (bits 8 ..; none is left when this is called) = the penalty so far (bits
// 0 .. 7), capped at `cap`; the penalty itself goes 0, 1, 2, 4, .. kNdBackoffVerdict.  (The runs sit in the upper bits so that
// "is a run being sat out" is one compare against a constant, as it was with a counter of its own.)
__device__ __forceinline__ uint32_t nd_backoff_refused(uint32_t bo, uint32_t cap)
{
    const uint32_t pen = bo & 0xffu;
    const uint32_t next = pen == 0u ? 1u : (pen < kNdBackoffVerdict ? pen * 2u : pen);
    return ((pen < cap ? pen : cap) << 8) | next;
}

// (counting build) The ONE-term NDZ body bound this kernel had before dc got a term of its own -- G = max(max|dz|, max|dc|) against
// the smallest 2^-26 lo_(j+m) over the growth (|2Z.re| + |2Z.im| + 1)(1 + 2^-10) per step, and the eighth arrival's own bound over it --
// for the statistics word that says what the second term buys (38).  `e` = the second companion from the entry the body starts at
// ({2Z.re, 2Z.im, the entry's own bound, -}), whose two-term bounds are not "never" (so e[0 .. 8] are usable).
__device__ __forceinline__ float ndz_one_term_bound(const float4 *__restrict__ e)
{
    float best = 0x1p60f, grow = 1.0f;
    for (uint32_t m = 0; m < 8; m++) {
        const float zr = __builtin_fabsf(e[m].x), zi = __builtin_fabsf(e[m].y);
        best = __builtin_fminf(best, __builtin_fminf(zr, zi) * 0x1p-26f / grow);
        grow *= (zr + zi + 1.0f) * (1.0f + 0x1p-10f);
    }
    return __builtin_fminf(best, e[8].z / grow) * (1.0f - 0x1p-10f);
}

// The untested body with the deferred verdict, SIXTEEN steps per body (round 4).  A wave that is alone on its SIMD -- the
// never-escaping pixels that decide C2's frame time, the last waves of a rank of an N-GPU split -- pays one L2 round trip per
// body: scalar loads return out of order, so the entries of a body can only be waited for all together, and the loads that
// warm the scalar cache for the next body are waited for with them.  Twice the steps per round trip: the body reads its
// entries in the COMPACT form -- 2Z alone, 8 bytes per entry (zs2: two s_load_dwordx16 for sixteen entries), and ONE
// 16-byte record (zqb) with the block bounds of its entries 3, 7, 11 and 15 -- instead of sixteen bytes per entry.
// Registers: entries E0 .. E15 in s[36:67] (E15 = s[66:67] is the entry the state is at when the body ends: the next
// body's first step reads it BEFORE the loads overwrite it), the four block bounds in s[72:75] (s75 = the bound of the
// state's entry at the loop's top), bases s[68:69] (zs2) and s[70:71] (zqb), `off` = 16 bytes per step as everywhere.
// State pairs, temporaries, the floor accumulator and the statuses as in FS_FAST_LOOP_FDU: 0 = stopped in front of a block
// that needs its tests / fewer than 16 steps left, 3 = a state below the floor (the caller repeats the run attempt with
// FS_FAST_LOOP_FL).  Blocks 2 .. 4 are tested in the second step of the block, before anything of the block is counted.
#define FS_FD16_TAIL(EC, ED)                                                                                        \
    FS_PK_F(FS_R2, EC) FS_FL_ACC("v50", "v51") FS_PK_MA(FS_R2) FS_FL_ACC("v52", "v53") FS_PK_MB(FS_R2)              \
    FS_PK_P FS_PK_A(FS_R3)                                                                                          \
    FS_PK_F(FS_R3, ED) FS_FL_ACC("v54", "v55") FS_PK_MA(FS_R3) FS_PK_MB(FS_R3) FS_PK_P FS_PK_A(FS_R0)

// The sixteen-step body as a TWO-STAGE PIPELINE (round 5).  Scalar loads return out of order behind one counter, so a wait is a
// wait for everything in flight -- but nothing says the wait has to follow the request: the body's entries live in two halves
// (E0 .. E7 in s[36:51] with the bounds of the entries 3 and 7 in s[72:73]; E8 .. E15 in s[52:67] with those of 11 and 15 in
// s[74:75]), and each half is requested while the OTHER one is being consumed -- the upper half at step 1 (right after the
// instruction that reads E15 of the body before), the next body's lower half at step 10 (right after the instructions that read
// E7 and the bound of entry 7) -- and waited for eight steps later, just before its first use, when it has long landed: the
// only thing in flight at either wait is the half requested eight steps ago.  A wave that is alone on its SIMD no longer
// stands still for an L2 round trip per body (C2's interior pixels: 4.7 M dependent steps; round 4's sixteen-step body with its
// warming loads measured ~30 ns per step against the ~19 ns of the step's dependent arithmetic).  Same registers as that body,
// statuses 0 and 3 as there (4: below).  The half requested past the end of a run is never used (the companion arrays carry 32
// entries of slack).
// The deferred floor verdict is taken PER BODY: the state a body starts from is kept (v[46:47], its step count in `cko`) once
// the verdict over the body before has passed, and a state below the floor sends the statement back to that checkpoint with
// status 3 -- the caller commits the certified steps and lets the per-trip loop (FS_FAST_LOOP_FL) find the failing trip in
// the sixteen steps that follow, instead of repeating the whole run with it (a 2048-step run that ends on a floor failure,
// which is how most runs of C2's never-escaping pixels end, was executed twice).
// The tests of the blocks INSIDE a body (its second to fourth) are deferred too (round 5): a wave that is alone on its SIMD
// issues in order, and `compare -> scalar or -> branch` makes it wait for the vector pipeline to drain at every block -- measured
// on the isolated loop (tools/microbench/lone_pace.hip) 20.7 ns per step with the three branches, 17.6 without, 11.0 for the
// arithmetic alone.  Each of those blocks leaves its verdict in v63 instead (positive = violated; it only grows):
//     max(max|w|, max|dc|) + Esh - bound, saturating (the "never" bound is the most negative integer),  and  max(..) - 2^14 (H;
//     max|dc| 2^-E <= 2^7 by the start condition, so taking the maximum with it changes nothing there)
// and the body's steps run on whatever comes.  ONE verdict per body, at the top of the next one (and on every way out): the floor
// accumulator v61 and v63 together; a violation of either sends the statement back to the body's checkpoint -- status 3 (floor
// alone: the caller commits the certified steps and lets the per-trip loop find the failing trip) or 4 (a block test: the
// caller takes the block in front of it through the tested form, as it does for status 0; the entry values it needs it reads
// itself).  What ran past a violated block test is discarded with the roll-back: nothing but registers was written.
// The first block of a body is treated the same way (blocks that need their tests are 0.1 % of the steps of C2's long pixels:
// a body run in vain in front of each costs nothing next to one more drain of the pipeline per body).
#define FS_FD16D_PAIR(EA, EB_, BW, WAIT, LOADS)                                                                     \
    FS_PK_F(FS_R0, EA) FS_FL_ACC("v48", "v49") FS_PK_MA(FS_R0)                                                      \
    "v_max3_f32 v62, |v48|, |v49|, %[imdc]\n\t"                                                                     \
    FS_PK_MB(FS_R0) FS_PK_P                                                                                         \
    "v_subrev_u32_e32 v45, 0x46800000, v62\n\t"                                                                     \
    FS_PK_A(FS_R1)                                                                                                  \
    "v_add_u32_e32 v62, v62, %[esh]\n\t" WAIT                                                                       \
    FS_PK_F(FS_R1, EB_)                                                                                             \
    "v_sub_i32 v62, v62, " BW " clamp\n\t"                                                                          \
    FS_PK_MA(FS_R1)                                                                                                 \
    "v_max3_i32 v63, v63, v62, v45\n\t"                                                                             \
    FS_PK_MB(FS_R1) FS_PK_P LOADS FS_PK_A(FS_R2)
#define FS_FAST_LOOP_FD16P                                                                                          \
    asm volatile(                                                                                                   \
        "v_mov_b32_e32 v61, 0x7f800000\n\t" /* the first body's lower half; every later body finds its own requested */ \
        "v_bfrev_b32_e32 v63, 1\n\t"                                                                                \
        "s_lshr_b32 %[oc], %[off], 1\n\t"                                                                           \
        "s_load_dwordx16 s[36:51], s[68:69], %[oc]\n\t"                                                             \
        "s_load_dwordx2 s[72:73], s[70:71], %[off]\n"                                                               \
        ".Lfp_loop_%=:\n\t" /* the verdict over the body before: floor (flr > the smallest part seen) or a block test */ \
        "v_sub_u32_e32 v45, %[flr], v61\n\t"                                                                        \
        FS_BT_DC_MAX "s_cmp_gt_u32 %[off], %[lim16]\n\t"                                                            \
        "v_max_i32_e32 v45, v45, v63\n\t"                                                                           \
        FS_BT_DC_ADD                                                                                                \
        "v_cmp_lt_i32_e32 vcc, 0, v45\n\t"                                                                          \
        "s_cbranch_vccnz .Lfp_redo_%=\n\t" /* sixteen steps left? */                                                \
        "s_cbranch_scc1 .Lfp_out_%=\n\t" /* the checkpoint: every state up to here is certified */                  \
        "v_mov_b32_e32 v46, v48\n\t"                                                                                \
        "v_mov_b32_e32 v47, v49\n\t"                                                                                \
        "s_mov_b32 %[cko], %[off]\n\t"                                                                              \
        "v_mov_b32_e32 v61, 0x7f800000\n\t" /* steps 1 .. 4 + the first block's verdict (s75, H) into v63 */        \
        FS_PK_F(FS_R0, "s[66:67]")                                                                                  \
        "v_sub_i32 v62, v62, s75 clamp\n\t"                                                                         \
        "v_subrev_u32_e32 v45, 0x46800000, v60\n\t"                                                                 \
        "s_waitcnt lgkmcnt(0)\n\t" /* the lower half has landed, the upper half is requested */                     \
        "s_lshr_b32 %[oc], %[off], 1\n\t"                                                                           \
        "s_load_dwordx16 s[52:67], s[68:69], %[oc] offset:0x40\n\t"                                                 \
        "s_load_dwordx2 s[74:75], s[70:71], %[off] offset:0x8\n\t"                                                  \
        FS_PK_MA(FS_R0)                                                                                             \
        "v_max_i32_e32 v63, v62, v45\n\t"                                                                           \
        FS_PK_MB(FS_R0) FS_PK_P FS_PK_A(FS_R1)                                                                      \
        FS_PK_F(FS_R1, "s[36:37]") FS_FL_ACC("v50", "v51") FS_PK_MA(FS_R1) FS_PK_MB(FS_R1) FS_PK_P FS_PK_A(FS_R2)   \
        FS_PK_F(FS_R2, "s[38:39]") FS_FL_ACC("v52", "v53") FS_PK_MA(FS_R2) FS_PK_MB(FS_R2) FS_PK_P FS_PK_A(FS_R3)   \
        FS_PK_F(FS_R3, "s[40:41]") FS_FL_ACC("v54", "v55") FS_PK_MA(FS_R3) FS_PK_MB(FS_R3) FS_PK_P FS_PK_A(FS_R0)   \
        /* steps 5 .. 8 */                                                                                          \
        FS_FD16D_PAIR("s[42:43]", "s[44:45]", "s72", "", "") FS_FD16_TAIL("s[46:47]", "s[48:49]")                   \
        /* steps 9 .. 12: the upper half has landed (step 10 reads E8); the next body's lower half is requested */   \
        FS_FD16D_PAIR("s[50:51]", "s[52:53]", "s73", "s_waitcnt lgkmcnt(0)\n\t",                                    \
                      "s_load_dwordx16 s[36:51], s[68:69], %[oc] offset:0x80\n\t"                                   \
                      "s_load_dwordx2 s[72:73], s[70:71], %[off] offset:0x100\n\t")                                 \
        FS_FD16_TAIL("s[54:55]", "s[56:57]")                                                                        \
        /* steps 13 .. 16 */                                                                                        \
        FS_FD16D_PAIR("s[58:59]", "s[60:61]", "s74", "", "") FS_FD16_TAIL("s[62:63]", "s[64:65]")                   \
        "s_add_u32 %[off], %[off], 0x100\n\t"                                                                       \
        FS_T_X("v48", "v49") FS_FL_ACC("v48", "v49") "s_branch .Lfp_loop_%=\n"                                      \
        ".Lfp_redo_%=:\n\t" /* back to the checkpoint (state, its max, step count): status 3 (floor) or 4 (a block test) */ \
        "v_mov_b32_e32 v48, v46\n\t"                                                                                \
        "v_mov_b32_e32 v49, v47\n\t"                                                                                \
        "v_cmp_lt_i32_e32 vcc, 0, v63\n\t"                                                                          \
        "s_mov_b32 %[off], %[cko]\n\t"                                                                              \
        FS_T_X("v46", "v47")                                                                                        \
        "s_mov_b32 %[st], 3\n\t"                                                                                    \
        "s_cbranch_vccz .Lfp_end_%=\n\t"                                                                            \
        "s_mov_b32 %[st], 4\n\t"                                                                                    \
        "s_branch .Lfp_end_%=\n"                                                                                    \
        ".Lfp_out_%=:\n\t" /* in front of a block that needs its tests, or of the last steps (the verdict has passed) */ \
        "s_mov_b32 %[st], 0\n"                                                                                      \
        ".Lfp_end_%=:\n\t"                                                                                          \
        "s_waitcnt lgkmcnt(0)"                                                                                      \
        : "+{v[48:49]}"(wv), "={v[50:51]}"(r1), "={v[52:53]}"(r2), "={v[54:55]}"(r3), "={v[56:57]}"(ts_),           \
          "={v[58:59]}"(ta_), "+{v60}"(mxS), "={v61}"(tn_), "={v62}"(tl_), "={v[46:47]}"(ck_), "={v45}"(th_),       \
          "={v63}"(va_), [st] "=&s"(st), "+{s75}"(pwi), "+{s[66:67]}"(zS), [off] "+s"(off), [oc] "=&s"(oc_),        \
          [cko] "=&s"(cko_)                                                                                         \
        : [se] "v"(sE2), [dc] "v"(dcs), [esh] "v"(Esh), [imdc] "v"(imdc), [lim16] "s"(lim16), "{s[68:69]}"(zpb2),   \
          "{s[70:71]}"(zqbp), [flr] "s"(kFloorBits)                                                                 \
        : "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50",  \
          "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65",  \
          "s72", "s73", "s74", "vcc", "scc")

// ------------------------------------------------------------------------------------------------
// LAv2, T = HDRFloat<float>: tuned perturbation loop.  Same prologue (AT + LA stages) and the same results, bit for
// bit, as k_lav2_hdr32; the perturbation loop (>99.9 % of the executed work at View 5) is restructured around what
// the CPU arithmetic actually does per step (measured with an instrumented oracle):
//   * 2Z+dz and Z'+dz are "orbit bigger, 0 <= exponent gap < 120" in 99.9 % of lane-steps; dz*cur+dc is "dz bigger".
//     A straight-line, branch-free step is executed speculatively under exactly those assumptions
//     (no 4-way exponent-alignment branches, no operand swaps) and committed only if EVERY running lane of the wave
//     met them (one ballot); otherwise the wave redoes that step with the generic functions of hdr_math.hpp.
//   * Reduce(z) before |z|^2 is skipped on the fast path: scaling both parts by the same power of two commutes with
//     IEEE multiply/add (no operand is near the denormal range there: the orbit part has |mantissa| >= 0.5), so
//     Reduce(|z|^2) gives the same {mantissa, exponent}.  The reduced z is only materialised on a rebase.
//   * Rebases (3.6e-4 per lane-step) and escapes leave the hot loop through cold branches.
//   * (exp, mantissa) pairs of reduced non-negative values are compared as one signed 64-bit key, which is the
//     lexicographic compareToBothPositiveReduced (HDRFloat.h:1150-1167) because IEEE bit patterns of non-negative
//     floats order like integers.
//   * The orbit entry of the *next* step is the Z' of this step: one 16-byte load per step instead of two.
namespace {

__device__ __forceinline__ float pow2_bits(int biased) { return __int_as_float(biased << 23); }

__device__ __forceinline__ long long key_of(float m, int e)
{
    return ((long long)e << 32) | (long long)(unsigned)__float_as_int(m);
}

// Reduce(norm_squared(c)) as a key; c is any complex whose larger part is a normal float.
__device__ __forceinline__ long long norm_key(float re, float im, int e)
{
    const float m = re * re + im * im; // >= +0
    const int bits = __float_as_int(m);
    const int fe = ((bits >> 23) & 0xff) - 127;
    const bool z = m == 0.0f;
    const int mm = z ? 0 : ((bits & 0x007FFFFF) | 0x3F800000);
    const int ee = (e << 1) + (z ? 0 : fe);
    return ((long long)ee << 32) | (long long)(unsigned)mm;
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imin3(int a, int b, int c)
{
    const int m = a < b ? a : b;
    return m < c ? m : c;
}

// 0x7F000000 - (f << 23) = the bits of 2^(127 - f), as one v_mad_i32_i24 (f < 2^8)
__device__ __forceinline__ int mad24_scale(int f)
{
    int r;
    const int k = -8388608;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(k), "s"(0x7F000000));
    return r;
}

// Same for a sum of squares already known to be a positive normal float (no zero special case).
__device__ __forceinline__ long long norm_key_nz(float m, int e)
{
    const int bits = __float_as_int(m);
    const int fe = ((bits >> 23) & 0xff) - 127;
    const int mm = (bits & 0x007FFFFF) | 0x3F800000;
    return ((long long)((e << 1) + fe) << 32) | (long long)(unsigned)mm;
}

} // namespace

// Steps per scaled run (a multiple of the 8-step body): a run's scale is fixed, and its lanes must have this many
// steps left before the orbit ends and before their iteration limit.  Measured on View 5 (C3 / C2, ms): 64: 69.9 / 385,
// 128: 68.6 / 390, 256: 68.0 / 372, 512: 68.2 / 380, 1024: 68.0 / 380, 4096: 78.9 / 561 (too few lanes qualify).
constexpr uint32_t kScaledChunk = 256;
static_assert(kScaledChunk % 8 == 0 && kScaledChunk >= 64, "a run is a whole number of 8-step bodies");

// Steps of the next scaled run: kScaledChunk when every (active) lane has that many left, else 64, else 16, else none --
// without the shorter runs the last 256 steps of every pass over the orbit (1.6 % of View 5's 16 046-entry orbit) fall to
// the exponent-tracking loop.
// Back-off of the scaled-run attempts: after an attempt that ended before its first step the wave takes this many careful
// steps more (1, 2, ... up to the cap) before it tries again; an attempt that got 8 steps or more resets it.  On C3 two
// thirds of the attempts of a wave (300 of 460) ended that way -- lanes near their escape, where dz is never small against
// the orbit -- each for the price of an entry, a trip and an exit.  Measured (C3 kernel ms / emulated 8-rank maximum): cap 0
// (no back-off) 60.3 / 10.27, 1: 57.7 / 9.81, 3: 56.5 / 9.41, 7: 55.8 / 9.36, 15: 55.5 / 9.13, 31: 56.1 / 9.28, 63: 55.4 / 9.17;
// doubling instead of counting up: no better; neither is waiting for a careful step that leaves every lane's dz 1 .. 4 binades
// below the orbit value it arrived at (57.3 .. 58.7).  Which steps run scaled changes no result.
constexpr uint32_t kScaledBackoffCap = 15;
// Steps of a hot run (k_lav2_hdr32_fast, see there) before the scale is re-centred.  Measured on C3 (kernel ms): 8: 50.2,
// 16: 49.75, 32: 49.7, 64: 49.5, 128 .. 1024: 49.5 - 49.6.
constexpr uint32_t kHotRunSteps = 64;

__device__ __forceinline__ uint32_t scaled_run_length(uint32_t left)
{
    if (__builtin_amdgcn_ballot_w64(left < kScaledChunk) == 0ull)
        return kScaledChunk;
    if (__builtin_amdgcn_ballot_w64(left < 64u) == 0ull)
        return 64u;
    return __builtin_amdgcn_ballot_w64(left < 16u) == 0ull ? 16u : 0u;
}

// ... and for the perturbation-only kernel (k_perturb_scalar): one longer tier in front.  A wave that is alone on its SIMD pays
// for every instruction of a run's entry and exit (and waits out their vector loads): at 256 steps per run they were 40 % of the
// time of C2's never-escaping pixels (tools/microbench/lone_pace.hip: the loop's own pace is 11.5 ns per step, the kernel's
// 21 - 31).  A run still ends where it has to: H, a floor or bound failure, a block that needs its tests at the very end.
constexpr uint32_t kPoChunk = 2048;
static_assert(kPoChunk % 16 == 0 && kPoChunk >= kScaledChunk && kPoChunk <= (1u << 20), "whole 16-step bodies; offsets stay 32-bit");
// Between the tiers: when every lane has as many steps left as the first one (the lanes of a never-escaping tile walk the orbit
// together), the run takes exactly those -- a pass over View 5's 16 046-entry orbit is then 8 runs instead of 17 (seven of 2048
// and the tail in one piece instead of 256 + 256 + ... + 16 + 16).  Multiples of four: the tested form behind the statement
// advances in four-step blocks.
__device__ __forceinline__ uint32_t scaled_run_length_po(uint32_t left)
{
    if (kPoChunk > kScaledChunk) {
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)left);
        const uint32_t want = (first < kPoChunk ? first : kPoChunk) & ~3u;
        if (want > kScaledChunk && __builtin_amdgcn_ballot_w64(left < want) == 0ull)
            return want;
    }
    return scaled_run_length(left);
}

// kLds (A/B variant, north_star "LDS staging of orbit segments shared across a wavefront"): in the scaled runs whose
// lanes share their orbit position, the entries reach the wave through LDS instead of the scalar cache.  Each wave owns
// two 1-KiB LDS buffers; one global_load_lds_dwordx4 (LDS-DMA: no VGPR destination, counted by vmcnt) brings the 64
// entries of the NEXT 64 steps while the current 64 are consumed with broadcast ds_read_b128 (every lane the same
// address; counted by lgkmcnt).  Two counters, in-order returns: a true software pipeline, which the scalar loads (one
// out-of-order counter) cannot be.  What it costs: the entries live in VGPRs (8 x 4 per body) and every ds_read writes
// 1 KiB of registers.  Measured against the scalar-cache path in DESIGN.md section 5.
// kGpuStage: the LA stage-validity test in the direction of the reference's GPU twin (FS_PARITY_CPU_GPUSTAGE) instead of
// the CPU function's (FS_PARITY_CPU) -- a template parameter so that the two parity modes are two kernels (they do very
// different work per frame, and a kernel trace then lists them separately).
// An upper bound, wave-uniform, of v over the ACTIVE lanes -- the largest value itself when a vote or two find it (the values of
// a wave's lanes, scales and dc, are a few binades apart at most), at most a few binades above it otherwise: each further trip
// adds a growing slack (1, 2, 4 ... 64 binades of a binary32 bit pattern), so the loop ends after a dozen trips at the latest whatever
// the lanes hold.  Votes instead of a reduction: nothing is written under a widened EXEC.  v <= 0x7f800000.
static __device__ __forceinline__ int wave_upper_bound_i32(int v)
{
    int m = __builtin_amdgcn_readfirstlane(v);
    int slack = 0;
    for (;;) {
        const uint64_t above = __builtin_amdgcn_ballot_w64(v > m);
        if (above == 0ull)
            return m;
        const long long next = (long long)__builtin_amdgcn_readlane(v, (int)__builtin_ctzll(above)) + slack;
        m = next > 0x7f800000ll ? 0x7f800000 : (int)next;
        slack = slack != 0 ? (slack < (64 << 23) ? slack * 2 : slack) : (1 << 23);
    }
}

