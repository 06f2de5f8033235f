// kernels_lav2_lit.hip -- the LITERAL LAv2 kernel for HDRFloat<float | double> (k_lav2_lit: the operation-by-operation A/B reference
// of the tuned kernels in kernels_lav2_hdr32.hip and kernels_hdr64.hip, and the kernel of the 64-bit counters and of the
// waypoint-resident orbits), the AT pass of the HDRFloat<double> frames and the test probe of the waypoint cursor.
// Compiled with -ffp-contract=off (see hdr_math.hpp).
//
// Parity target is a reference *CPU* RenderAlgorithm function (cited at the kernel); the decomposition is this project's own: one
// lane per (sub)pixel, reference orbit pre-converted once per upload (kernels_orbit_prep.hip) into the complex form the CPU loop
// rebuilds on every access.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/fs_layout.h"
#include "hdr_math.hpp"
#include "at_math.hpp"
#include "kernels.h"
#include "kernel_common.hpp"
#include "launch_dispatch.hpp"
#include "lav2_common.hpp"
#include "seq_orbit.hpp"

using namespace fs;

// ------------------------------------------------------------------------------------------------
// The waypoint cursor (SeqOrbit<F, PosT>: sequential access to a SimpleCompression orbit that stays compressed in HBM) is in
// seq_orbit.hpp, shared with the Feature Finder's evaluator.
namespace {

// test hook (fs_seq_cursor_probe): one lane seeks to `start` and walks n entries on; out[k] = the value at start + k
template <class F, class PosT>
__global__ void k_seq_cursor_probe(const void *wp, uint32_t n_wp, hreal<F> cx, hreal<F> cy, uint64_t start, uint32_t n,
                                   hcplx<F> *out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    SeqOrbit<F, PosT> seq;
    seq.wp = (const typename FsWaypoints<F>::Rec *)wp;
    seq.n_wp = n_wp;
    seq.cx = cx, seq.cy = cy;
    seq.seek((PosT)start);
    for (uint32_t k = 0; k < n; k++) {
        out[k] = seq.value();
        seq.step();
    }
}

} // namespace

// ------------------------------------------------------------------------------------------------
// LAv2, T = HDRFloat<float>.  CPU twin: Fractal::CalcCpuPerturbationFractalLAV2<uint32_t,float,Disable>
// (Fractal.cpp:2545-2678) with LAReference::getLA / isLAStageInvalid (LAReference.cpp:1076-1134),
// LAInfoDeep::Prepare / Evaluate (LAInfoDeep.h:395-420), ATInfo::PerformAT (ATInfo.h:155-188).
// Replaces mandel_1xHDR_float_perturb_lav2 (FractalSharkGpuLib/LAKernel.cuh:3-315).
// IterT = the reference's IterType for the COUNTERS (LAKernel.cuh:3): uint32_t, or uint64_t for iteration caps of 2^32 and
// above (iterations, the cap, the AT iteration count and the skipped-iteration product are then 64-bit; table step
// lengths and indices stay 32-bit -- an orbit or table with 2^32 entries would not fit any device).
// kSeq: the orbit is a compressed one that stays compressed (A.wp): every orbit value comes from a SeqOrbit cursor.
template <class F, int Mode, bool kStats, class IterT = uint32_t, bool kSeq = false>
__global__ void __launch_bounds__(256) k_lav2_lit(FsLav2ArgsT<F> A)
{
    // The float instantiation is the operation-by-operation A/B reference of the tuned kernel and keeps the literal AT
    // loop; the double instantiation is the production HDRFloat<double> kernel and uses the steady-state AT loop.
    constexpr bool kFastAT = sizeof(F) == 8;
    // 64-bit POSITIONS go with the waypoint-resident orbit and 64-bit counters (see SeqOrbit); every other instantiation
    // keeps 32-bit ones (an expanded orbit of 2^32 entries does not fit a device)
    constexpr bool kWidePos = kSeq && sizeof(IterT) == 8;
    using PosT = std::conditional_t<kWidePos, uint64_t, uint32_t>;
    using LaRec = typename FsDev<F>::LA;
    using LaRec64 = typename FsLaU64<F>::T;
    // the table's records: the narrowed (uint32_t) ones, or the reference's uint64_t records as they are (A.la_u64) -- the
    // two layouts agree up to StepLength, so the coefficients are read through the narrow type either way
    const bool la64 = kWidePos && A.la_u64 != 0u;
    auto la_rec = [&](uint64_t idx) -> const LaRec * {
        return la64 ? (const LaRec *)((const LaRec64 *)(const void *)A.las + idx) : A.las + idx;
    };
    auto la_step_length = [&](const LaRec *p) -> IterT {
        return la64 ? (IterT)((const LaRec64 *)(const void *)p)->StepLength : (IterT)p->StepLength;
    };
    auto la_next_stage = [&](const LaRec *p) -> PosT {
        return la64 ? (PosT)((const LaRec64 *)(const void *)p)->NextStageLAIndex : (PosT)p->NextStageLAIndex;
    };
    uint32_t X, L;
    if (A.pixel_order)
        ordered_pixel(A.frame, A.pixel_order, X, L);
    else
        tile_pixel(X, L);
    uint64_t c_at = 0, c_la = 0, c_pt = 0, c_px = 0, c_at_exec = 0; // (c_at_exec: AT iterations actually run -- the cycle search of at_perform spares the rest)
    uint32_t px_cost = 0; // AT iterations this pixel ran (FsLav2ArgsT::pixel_cost)
    uint64_t c_at_own = 0; // AT iterations this pixel needs by itself (what the AT pass of its own runs for it: statistics word 6)
    const bool in_buffer = X < A.frame.width && L < A.frame.local_rows;
    const uint32_t Y = in_buffer ? global_row(A.frame, L) : 0xFFFFFFFFu;
    const bool live = in_buffer && Y < A.frame.height;
    if (live) {
        c_px = 1;
        const IterT n_iterations = sizeof(IterT) == 8 ? (IterT)(((uint64_t)A.n_iterations_hi << 32) | A.n_iterations)
                                                      : (IterT)A.n_iterations;
        hreal<F> deltaReal, deltaImaginary;
        pixel_delta<F>(A.coords, X, Y, deltaReal, deltaImaginary);
        const hcplx<F> DeltaSub0 = hc_from_hr(deltaReal, deltaImaginary);
        hcplx<F> DeltaSubN = hc_from_native<F>(F(0), F(0)); // {0,0}: zero with exponent 0 (Fractal.cpp:2565)
        IterT iterations = 0;

        bool at_done = false;
        if constexpr (Mode != FS_MODE_PO && std::is_same<F, double>::value && sizeof(IterT) == 4 && !kSeq) {
            if (A.at_res) { // PerformAT ran in its own pass (fsk_at_pass64): its result instead of the iteration
                const FsAtRes ar = A.at_res[(size_t)L * A.frame.rounded_width + X];
                at_done = true;
                if (ar.i != 0xFFFFFFFFu) {
                    DeltaSubN = hcplx<F>{ar.re, ar.im, ar.e};
                    iterations = (IterT)ar.i * (IterT)A.at.StepLength;
                }
            }
        }
        if (Mode != FS_MODE_PO && !at_done) {
            if (A.la_valid && A.use_at && hr_cmp_pos(hc_cheb(DeltaSub0), ldr(A.at.ThresholdC)) <= 0) {
                const IterT at_step = kWidePos ? (IterT)(((uint64_t)A.at_step_hi << 32) | A.at.StepLength) : (IterT)A.at.StepLength;
                const IterT ATMaxIt = n_iterations / at_step;
                hcplx<F> c = hc_add(hc_mul(DeltaSub0, ldc(A.at.CCoeff)), ldc(A.at.RefC));
                hc_reduce(c);
                hcplx<F> z;
                IterT i, i_exec = 0, i_own = 0;
                if (kFastAT) {
                    at_perform<F, IterT>(c, ldr(A.at.SqrEscapeRadius), ATMaxIt, z, i, &i_exec, &i_own);
                    px_cost = i_own > (IterT)0xFFFFFu ? 0xFFFFFu : (uint32_t)i_own;
                } else {
                    z = hc_zero<F>();
                    const hreal<F> esc = ldr(A.at.SqrEscapeRadius);
                    for (i = 0; i < ATMaxIt; i++) {
                        hreal<F> nsq = hc_norm2(z);
                        hr_reduce(nsq);
                        if (hr_cmp_pos(nsq, esc) > 0)
                            break;
                        z = hc_add(hc_mul(z, z), c);
                    }
                }
                hcplx<F> dz = hc_mul(z, ldc(A.at.InvZCoeff));
                hc_reduce(dz);
                DeltaSubN = dz;
                iterations = i * at_step;
                if (kStats) {
                    c_at = i;
                    c_at_exec = kFastAT ? (uint64_t)i_exec : (uint64_t)i;
                    c_at_own = kFastAT ? (uint64_t)i_own : (uint64_t)i;
                }
            }
        }

        PosT RefIteration = 0;
        const PosT MaxRefIteration = (kWidePos ? (PosT)(((uint64_t)A.orbit_count_hi << 32) | A.orbit_count) : (PosT)A.orbit_count) - 1;
        const PosT period = kWidePos ? (PosT)(((uint64_t)A.period_hi << 32) | A.period) : (PosT)A.period;
        // complex0 before the LA stages is dead in the CPU function (only its norm was read, into a variable
        // that is overwritten before use), so it is not materialised; the RefIteration %= period side effect
        // (Fractal.cpp:2590-2591) is kept.
        if (iterations != 0 && !(RefIteration < MaxRefIteration) && period != 0)
            RefIteration = RefIteration % period;

        if (Mode != FS_MODE_PO) {
            uint32_t CurrentLAStage = A.la_valid ? A.stage_count : 0;
            const hreal<F> dcCheb = hc_cheb(DeltaSub0);
            while (CurrentLAStage > 0) {
                CurrentLAStage--;
                const uint32_t LAIndex = A.stages[CurrentLAStage].LAIndex;
                {
                    const int cmp = hr_cmp_pos(dcCheb, ldr(la_rec(LAIndex)->LAThresholdC));
                    const bool invalid = A.parity == FS_PARITY_LITERAL ? (cmp < 0) : (cmp >= 0);
                    if (invalid)
                        continue;
                }
                const uint32_t MacroItCount = A.stages[CurrentLAStage].MacroItCount;
                PosT j = RefIteration;
                // (round 4) the Ref of record j + 1, read for the rebase test of step j, is the Ref step j + 1 starts from:
                // one load of it per step, not two, unless the test reset j
                hcplx<F> RefJ = hc_zero<F>();
                if (iterations < n_iterations)
                    RefJ = ldc(la_rec((uint64_t)LAIndex + j)->Ref);
                while (iterations < n_iterations) {
                    const LaRec *LAj = la_rec((uint64_t)LAIndex + j);
                    const IterT l = la_step_length(LAj);
                    bool unusable = true;
                    hcplx<F> newDz = hc_zero<F>();
                    if (iterations + l <= n_iterations) {
                        newDz = hc_mul(DeltaSubN, hc_add(hc_mul2(RefJ), DeltaSubN));
                        hc_reduce(newDz);
                        unusable = hr_cmp_pos(hc_cheb(newDz), ldr(LAj->LAThreshold)) >= 0;
                    }
                    if (unusable) {
                        RefIteration = la_next_stage(LAj);
                        break;
                    }
                    iterations += l;
                    if (kStats)
                        c_la++;
                    DeltaSubN = hc_add(hc_mul(newDz, ldc(LAj->ZCoeff)), hc_mul(DeltaSub0, ldc(LAj->CCoeff)));
                    const hcplx<F> RefN = ldc(la_rec((uint64_t)LAIndex + j + 1)->Ref);
                    const hcplx<F> complex0 = hc_add(RefN, DeltaSubN);
                    j++;
                    const hreal<F> lhs = hr_reduced(hc_cheb(complex0));
                    const hreal<F> rhs = hr_reduced(hc_cheb(DeltaSubN));
                    if (hr_cmp_pos(lhs, rhs) < 0 || j >= MacroItCount) {
                        DeltaSubN = complex0;
                        j = 0;
                        RefJ = ldc(la_rec((uint64_t)LAIndex)->Ref);
                    } else {
                        RefJ = RefN;
                    }
                }
                if (iterations >= n_iterations)
                    break;
            }
        }

        const IterT it_la = iterations; // (the perturbation steps of this pixel = its final count - this)
        if (Mode != FS_MODE_LAO) {
            const hreal<F> TwoFiftySix = hreal<F>{F(1), 8};
            const typename FsDev<F>::Z *__restrict__ zr = A.zref;
            SeqOrbit<F, PosT> seq;
            if constexpr (kSeq) {
                seq.wp = (const typename FsWaypoints<F>::Rec *)A.wp;
                seq.n_wp = A.n_wp;
                seq.cx = ldr(A.cxLow), seq.cy = ldr(A.cyLow);
                if (iterations < n_iterations)
                    seq.seek(RefIteration); // SeqWorkspace(results, RefIteration)
            }
            // (round 4) Two things the reference's loop does per step are not done per step here, with the same results:
            // the orbit entry a step arrives at is the entry the next step leaves from -- one load per step, not two, unless
            // a rebase moved the index; and Reduce(z) before |z|^2 only re-labels z -- both parts scaled by the same power of
            // two, which commutes with the squares and their sum (the larger part of z is an O(1) mantissa: nothing comes
            // near the ends of the range) -- so the reduced norm is the same and z is reduced only where it is stored, on a
            // rebase.
            hcplx<F> Zhere = hc_zero<F>();
            if constexpr (!kSeq) {
                if (iterations < n_iterations)
                    Zhere = zref_at(zr, (uint32_t)RefIteration);
            }
            for (; iterations < n_iterations; iterations++) {
                hcplx<F> cur;
                if constexpr (kSeq)
                    cur = seq.value();
                else
                    cur = Zhere;
                cur = hc_mul2(cur);
                cur = hc_add(cur, DeltaSubN);
                DeltaSubN = hc_mul(DeltaSubN, cur);
                DeltaSubN = hc_add(DeltaSubN, DeltaSub0);
                hc_reduce(DeltaSubN);
                if (kStats)
                    c_pt++;
                RefIteration++;
                hcplx<F> Znext;
                if constexpr (kSeq) {
                    seq.step(); // GetIterSeq
                    Znext = seq.value();
                } else {
                    Znext = zref_at(zr, (uint32_t)RefIteration);
                    Zhere = Znext;
                }
                hcplx<F> complex0 = hc_add(Znext, DeltaSubN);
                const hreal<F> normSquared = hr_reduced(hc_norm2(complex0));
                const hreal<F> DeltaNormSquared = hr_reduced(hc_norm2(DeltaSubN));
                if (hr_cmp_pos(normSquared, TwoFiftySix) > 0)
                    break;
                if (hr_cmp_pos(normSquared, DeltaNormSquared) < 0 || RefIteration >= MaxRefIteration) {
                    hc_reduce(complex0);
                    DeltaSubN = complex0;
                    RefIteration = 0;
                    if constexpr (kSeq)
                        seq.seek(0); // a new SeqWorkspace at the start of the orbit
                    else
                        Zhere = zref_at(zr, 0u);
                }
            }
        }
        store_iter(A.out, A.frame, L, X, iterations);
        if (A.pixel_cost) {
            // AT iterations first, perturbation steps second: the two phases run one after the other and a wave pays the
            // longest lane of each, so pixels should agree in both (a single sum puts a pixel that iterates long and steps
            // little next to one that does the opposite)
            const uint64_t pt = (uint64_t)(iterations - it_la);
            A.pixel_cost[(size_t)L * A.frame.rounded_width + X] = (px_cost << 12) | (pt > 0xFFFull ? 0xFFFu : (uint32_t)pt);
        }
    }
    if (kStats) {
        add_stats(A.stats, c_at, c_la, c_pt, c_px);
        // statistics word 5 (this kernel has no careful steps to report there): AT iterations executed
        uint64_t e = c_at_exec;
        for (int off = 32; off > 0; off >>= 1)
            e += __shfl_down(e, off);
        uint64_t o = c_at_own;
        for (int off = 32; off > 0; off >>= 1)
            o += __shfl_down(o, off);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd((unsigned long long *)&A.stats[5], (unsigned long long)e);
            atomicAdd((unsigned long long *)&A.stats[6], (unsigned long long)o);
        }
    }
}

// PerformAT of every pixel in a pass of its own (see FsLav2ArgsT::at_res): the same pixel delta, the same isValid test, the same
// at_perform and the same dz = z * InvZCoeff as k_lav2_lit<double> -- stored instead of used.
__global__ void __launch_bounds__(256) k_at_pass64(FsLav2ArgsT<double> A)
{
    using F = double;
    uint32_t X, L;
    if (A.pixel_order)
        ordered_pixel(A.frame, A.pixel_order, X, L);
    else
        tile_pixel(X, L);
    const bool in_buffer = X < A.frame.width && L < A.frame.local_rows;
    const uint32_t Y = in_buffer ? global_row(A.frame, L) : 0xFFFFFFFFu;
    if (!(in_buffer && Y < A.frame.height))
        return;
    hreal<F> deltaReal, deltaImaginary;
    pixel_delta<F>(A.coords, X, Y, deltaReal, deltaImaginary);
    const hcplx<F> DeltaSub0 = hc_from_hr(deltaReal, deltaImaginary);
    FsAtRes out{0.0, 0.0, 0, 0xFFFFFFFFu};
    uint32_t own = 0;
    if (A.la_valid && A.use_at && hr_cmp_pos(hc_cheb(DeltaSub0), ldr(A.at.ThresholdC)) <= 0) {
        const uint32_t ATMaxIt = A.n_iterations / A.at.StepLength;
        hcplx<F> c = hc_add(hc_mul(DeltaSub0, ldc(A.at.CCoeff)), ldc(A.at.RefC));
        hc_reduce(c);
        hcplx<F> z;
        uint32_t i, i_exec = 0, i_own = 0;
        at_perform<F, uint32_t>(c, ldr(A.at.SqrEscapeRadius), ATMaxIt, z, i, &i_exec, &i_own);
        hcplx<F> dz = hc_mul(z, ldc(A.at.InvZCoeff));
        hc_reduce(dz);
        out = FsAtRes{dz.re, dz.im, dz.e, i};
        own = i_own;
    }
    const size_t idx = (size_t)L * A.frame.rounded_width + X;
    A.at_res[idx] = out;
    if (A.at_cost)
        A.at_cost[idx] = own;
    if (A.pixel_cost) // the frame's own order (round 6): the AT iteration count is the leading part of the pixel's final count
        A.pixel_cost[idx] = out.i == 0xFFFFFFFFu ? 0u : out.i;
}

// ------------------------------------------------------------------------------------------------
// Host-callable launchers (called from renderer_launch.cpp and kernels_lav2_hdr32.hip through kernels.h).
void fsk_at_pass64(const FsLav2ArgsT<double> &A, hipStream_t s)
{
    hipLaunchKernelGGL(k_at_pass64, fsl::tile_grid(A.frame), dim3(256), 0, s, A);
}

// The one launcher of k_lav2_lit.  This kernel is the exception to the rule of launch_dispatch.hpp: it counts steps with 64-bit
// counters and on a waypoint-resident orbit too -- every combination is built but <kSeq, uint64_t> with step counters.
template <class F, bool kSeq> static void launch_lit(const FsLav2ArgsT<F> &A, int mode, bool stats, bool wide, hipStream_t s)
{
    const dim3 g = fsl::tile_grid(A.frame), b(256);
    fsl::with_mode(mode, [&](auto m) {
        fsl::with_bool(wide, [&](auto w) {
            fsl::with_bool(stats && !(kSeq && wide), [&](auto st) {
                constexpr bool kWide = decltype(w)::value, kStats = decltype(st)::value;
                if constexpr (!(kSeq && kWide && kStats))
                    hipLaunchKernelGGL((k_lav2_lit<F, decltype(m)::value, kStats, fsl::iter_t<kWide>, kSeq>), g, b, 0, s, A);
            });
        });
    });
}

// the literal HDRFloat<float> kernel (FS_VARIANT_LITERAL of fsk_lav2_hdr32, kernels_lav2_hdr32.hip)
void fsk_lav2_lit32(const FsLav2Args32 &A, int mode, bool stats, hipStream_t s) { launch_lit<float, false>(A, mode, stats, false, s); }
void fsk_lav2_hdr64(const FsLav2ArgsT<double> &A, int mode, bool stats, hipStream_t s)
{
    launch_lit<double, false>(A, mode, stats, false, s);
}
void fsk_lav2_wide(const FsLav2Args32 &A, int mode, bool stats, hipStream_t s) { launch_lit<float, false>(A, mode, stats, true, s); }
void fsk_lav2_wide(const FsLav2ArgsT<double> &A, int mode, bool stats, hipStream_t s)
{
    launch_lit<double, false>(A, mode, stats, true, s);
}
void fsk_lav2_seq(const FsLav2Args32 &A, int mode, bool stats, hipStream_t s)
{
    launch_lit<float, true>(A, mode, stats, A.frame.wide != 0u, s);
}
void fsk_lav2_seq(const FsLav2ArgsT<double> &A, int mode, bool stats, hipStream_t s)
{
    launch_lit<double, true>(A, mode, stats, A.frame.wide != 0u, s);
}

void fsk_seq_cursor_probe(bool is64, bool wide_pos, const void *wp, uint32_t n_wp, const void *cx, const void *cy,
                          uint64_t start, uint32_t n, void *out, hipStream_t s)
{
    auto launch = [&](auto f, const auto *x, const auto *y) { // f: 0.0f or 0.0, the float type of the orbit
        using F = decltype(f);
        const hreal<F> hx{x->m, x->e}, hy{y->m, y->e};
        fsl::with_bool(wide_pos, [&](auto w) {
            hipLaunchKernelGGL((k_seq_cursor_probe<F, fsl::iter_t<decltype(w)::value>>), dim3(1), dim3(64), 0, s, wp, n_wp, hx, hy,
                               start, n, (hcplx<F> *)out);
        });
    };
    if (is64)
        launch(0.0, (const fs_real_hdr64 *)cx, (const fs_real_hdr64 *)cy);
    else
        launch(0.0f, (const fs_real_hdr32 *)cx, (const fs_real_hdr32 *)cy);
}
