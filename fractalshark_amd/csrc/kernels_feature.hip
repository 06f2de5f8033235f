// kernels_feature.hip -- the Feature Finder's perturbation evaluator (fs_feature_eval): one lane per candidate.
//
// Restates, operation for operation, in the arithmetic of hdr_math.hpp (HDRFloat<float | double>):
//   FeatureFinder::Evaluate_PT<true | false>                 FeatureFinder.cpp:1757-1958
//   PeriodicityPP::Init / CheckPeriodicity                   FeatureFinder.cpp:1471-1534
//   FeatureFinder::Evaluate_PeriodResidualAndDzdc_Direct     FeatureFinder.cpp:1661-1711   (feature_steps.hpp)
//   PTEvaluator::Eval (PT, then Direct when a fixed-period PT evaluation escapes)  FeatureFinder.cpp:2313-2354
// Points the reference fixes and this file keeps: escape radius^2 4096; the rebase test (refIteration >= count - 1 or
// |z|^2 < |dz|^2) comes before the escape test; zcoeff and dzdc are advanced with the previous step's z; every product with the
// unit scaling factor (scaleExp = 0) is performed, because it clamps exponents and reduces; C{} / T{} are the default
// constructors, zero with exponent MIN_BIG_EXPONENT (HDRFloatComplex.h:121-126, HDRFloat.h:200-204).
//
// A candidate may need up to 2^31 steps (and the Direct fallback as many again), so the evaluation runs in bounded slices: each
// launch advances every unfinished lane by at most `slice` steps and keeps its state in FsFeatLane records between launches.
// All lanes start at orbit position 0 and stay in lockstep until their first rebase; while the wave's active lanes agree on the
// position (a ballot vote), the two orbit entries of the step are read once for the wave through the scalar cache, else each
// lane loads its own.
//
// fs_feature_eval_resident on a waypoint-resident orbit (k_feature_step_seq): the same step loop, with the two orbit entries of a
// step taken from a decompression cursor per lane (seq_orbit.hpp) in place of the expanded array.  The cursor sits at the lane's
// orbit position; stepping it once yields the entry the step arrives at, a rebase rewinds it to waypoint 0, and its state is
// part of the lane record (FsFeatSeqLane), so a slice goes on where the last one stopped without seeking.  Positions are as
// wide as the IterType, as the reference's are (Perturb.cuh:21-23, 202-203).
#include "feature_steps.hpp"
#include "seq_orbit.hpp"

using namespace fs;
using namespace fsfeat;

namespace {

// Orbit entry i as a complex.  P = a global pointer (each lane its own entry: vector loads) or a constant-address-space one with a
// wave-uniform index (one scalar load for the wave); fields read one by one (an address-space-qualified record cannot be copied
// whole in the host pass).
template <class Z> struct OrbitRead;
template <> struct OrbitRead<float4> { // {re, im, bitcast(exp), -}
    template <class P> static __device__ __forceinline__ hcplx32 at(P z, uint32_t i)
    {
        return hcplx32{z[i].x, z[i].y, __float_as_int(z[i].z)};
    }
};
template <> struct OrbitRead<FsZ64> {
    template <class P> static __device__ __forceinline__ hcplx64 at(P z, uint32_t i) { return hcplx64{z[i].re, z[i].im, z[i].e}; }
};

// Evaluate_PT's set-up (:1774-1827) and PeriodicityPP::Init (:1478-1496); a candidate that fails it is finished here
// (rejected in find mode, handed to the Direct loop in fixed mode, as PTEvaluator::Eval does).
// Start = what a lane record holds besides: nothing (NoCursor), or the cursor at waypoint 0 (CursorAtStart).
struct NoCursor {
    template <class Lane> __device__ __forceinline__ void operator()(Lane &) const {}
};
template <class F, class PosT> struct CursorAtStart {
    const typename FsWaypoints<F>::Rec *wp;
    uint32_t n_wp;
    __device__ __forceinline__ void operator()(FsFeatSeqLane<F, PosT> &s) const
    {
        SeqOrbit<F, PosT> seq;
        seq.wp = wp;
        seq.n_wp = n_wp;
        seq.rewind();
        s.zx = seq.zx, s.zy = seq.zy;
        s.next = seq.next;
        s.next_index = seq.next_index;
    }
};

template <class F, class Lane, class Start>
__global__ void __launch_bounds__(64) k_feature_init(const typename FsFeatRec<F>::In *__restrict__ in,
                                                      Lane *__restrict__ st, typename FsFeatRec<F>::Out *__restrict__ out,
                                                      uint64_t n, int find, hreal<F> R, uint64_t max_iters, uint64_t count,
                                                      Start start)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const auto inp = in[i];
    Lane s;
    start(s);
    s.dc = hcplx<F>{inp.dc.re, inp.dc.im, inp.dc.e};
    s.c = hcplx<F>{inp.c.re, inp.c.im, inp.c.e};
    s.period = inp.period;
    s.z = hc_zero<F>();
    s.dz = hc_zero<F>();
    s.dzdc = hc_zero<F>();
    s.zcoeff = hc_zero<F>();
    s.sqr_r = hr_zero<F>();
    s.sqr_scale = hr_zero<F>();
    s.step = 0;
    s.ref = 0;
    s.cap = find ? max_iters : inp.period;
    s.phase = kPhasePT;
    bool ok = count >= 2 && s.cap >= 1;
    if (ok && find) {
        hr_reduce(R);
        if (hr_cmp_pos(R, hr_zero<F>()) <= 0) {
            ok = false;
        } else {
            // PeriodicityPP::Init: R^2 and (0.25)^2, each reduced
            const hreal<F> near1 = hr_from_number<F>(F(0.25));
            s.sqr_r = hr_reduced(hr_mul(R, R));
            s.sqr_scale = hr_reduced(hr_mul(near1, near1));
        }
    }
    if (!ok) {
        if (find) {
            s.phase = kPhaseDone;
            out[i] = typename FsFeatRec<F>::Out{};
        } else {
            s.phase = kPhaseDirect;
            s.cap = inp.period;
        }
    }
    st[i] = s;
}

// How the two orbit entries of a step arrive.  An Orbit knows the lane's position: pair() yields the entries at the position
// and behind it and moves the position on by one, at_end() is the reference's refIteration >= count - 1, rebase() goes back to 0.
//
// The expanded orbit: the position is the lane record's `ref`, held here while a slice runs.
template <class F> struct ExpandedOrbit {
    using Z = typename FsDev<F>::Z;
    const Z *__restrict__ zref;
    uint32_t count;
    uint32_t ref;

    __device__ __forceinline__ void pair(hcplx<F> &zr, hcplx<F> &zr1)
    {
        typedef const __attribute__((address_space(4))) Z *ZC;
        // once for the wave when its PT lanes agree on the position
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)ref);
        if (__builtin_amdgcn_ballot_w64(ref == first) == __builtin_amdgcn_ballot_w64(true)) {
            // (through the constant address space: said explicitly, or the compiler folds the two arms into one vector load
            // of a per-lane selected index)
            const ZC zc = (ZC)(uintptr_t)zref;
            zr = OrbitRead<Z>::at(zc, first);
            zr1 = OrbitRead<Z>::at(zc, first + 1);
        } else {
            zr = OrbitRead<Z>::at(zref, ref);
            zr1 = OrbitRead<Z>::at(zref, ref + 1);
        }
        ref++;
    }
    __device__ __forceinline__ bool at_end() const { return ref >= count - 1; }
    __device__ __forceinline__ void rebase() { ref = 0; }
};

// The waypoint-resident orbit: the position is the cursor's, whose state the lane record carries between slices.  The cursor
// never steps past the last entry: a lane that arrives at count - 1 rebases in the same step (at_end), before the next pair().
// rebase() is seek(0) without the binary search.
template <class F, class PosT> struct WaypointOrbit {
    SeqOrbit<F, PosT> seq;
    PosT count;

    __device__ __forceinline__ void pair(hcplx<F> &zr, hcplx<F> &zr1)
    {
        zr = seq.value();
        seq.step();
        zr1 = seq.value();
    }
    __device__ __forceinline__ bool at_end() const { return seq.idx >= count - 1; }
    __device__ __forceinline__ void rebase() { seq.rewind(); }
};

// Up to `slice` steps of one candidate (every lane of the wave calls it).  IterT = the reference's IterType: the width periods
// are counted at.  Lane = FsFeatLane<F> / FsFeatSeqLane<F, PosT>; the orbit position is the Orbit's, not the lane's `ref`.
// (The lane goes in and comes out by value: taken by reference, k_feature_step<double, ..> comes out of the compiler with 53
// scalar registers in place of the 55 it has with this loop written out in the kernel; by value the four instantiations have
// the registers they had.)
template <class F, class IterT, class Lane, class Orbit>
__device__ __forceinline__ Lane feature_slice(Lane s, Orbit &orbit, typename FsFeatRec<F>::Out *out, uint64_t i,
                                              int find, uint32_t slice)
{
    const hreal<F> zero = hr_zero<F>();
    const hreal<F> one = hr_from_number<F>(F(1));
    const hreal<F> two = hr_from_number<F>(F(2));
    const hreal<F> escape2 = hr_from_number<F>(F(4096));
    // scaleExp = 0: ScalingFactor = InvScalingFactor = HdrLdexp(one, 0) = {1, 0}; C(s, T{}) of it; InvScale2 = reduce(1 * 1)
    const hcplx<F> scaleC = hc_from_hr(one, zero);
    const hcplx<F> invScaleC = hc_from_hr(one, zero);
    const hreal<F> invScale2 = hr_reduced(hr_mul(one, one));
    const hcplx<F> oneC = hc_reduced(hc_from_hr(one, zero));

    for (uint32_t k = 0; k < slice; ++k) {
        if (__ballot(s.phase != kPhaseDone) == 0)
            break;
        if (s.phase == kPhasePT) {
            // Evaluate_PT loop body, :1829-1915
            if (s.step == 0)
                s.zcoeff = scaleC;
            else
                s.zcoeff = hc_mul(s.zcoeff, hc_mul_real(s.z, two));
            hc_reduce(s.zcoeff);
            s.dzdc = hc_add(hc_mul(s.dzdc, hc_mul_real(s.z, two)), scaleC);
            hc_reduce(s.dzdc);

            // the orbit entries at refIteration and refIteration + 1; the position is refIteration + 1 afterwards
            hcplx<F> zr, zr1;
            orbit.pair(zr, zr1);

            s.dz = hc_add(hc_mul(s.dz, hc_add(zr, s.z)), s.dc);
            hc_reduce(s.dz);
            s.z = hc_add(zr1, s.dz);
            hc_reduce(s.z);

            const hreal<F> dzNorm = hr_reduced(hc_norm2(s.dz));
            const hreal<F> zNorm = hr_reduced(hc_norm2(s.z));
            if (orbit.at_end() || hr_cmp_pos(zNorm, dzNorm) < 0) {
                s.dz = hc_reduced(s.z);
                orbit.rebase();
            }
            s.step++;

            if (hr_cmp_pos(zNorm, escape2) > 0) {
                if (find) {
                    s.phase = kPhaseDone;
                    out[i] = typename FsFeatRec<F>::Out{};
                } else {
                    // PTEvaluator::Eval<false>: PT failed, DIRECT at the same period
                    s.phase = kPhaseDirect;
                    s.cap = s.period;
                    s.step = 0;
                    s.z = hc_zero<F>();
                    s.dzdc = hc_zero<F>();
                    s.zcoeff = hc_zero<F>();
                }
                continue;
            }

            if (find) {
                const hreal<F> dzdcNormTrue = hr_reduced(hr_mul(hr_reduced(hc_norm2(s.dzdc)), invScale2));
                // PeriodicityPP::CheckPeriodicity
                const hreal<F> rhs = hr_reduced(hr_mul(s.sqr_r, dzdcNormTrue));
                if (hr_cmp_pos(zNorm, rhs) < 0) {
                    store_out<F>(out[i], FS_FEATURE_OK, (uint64_t)(IterT)s.step, hc_reduced(s.z),
                                 hc_reduced(hc_mul(s.dzdc, invScaleC)), hc_reduced(hc_mul(s.zcoeff, invScaleC)), zNorm);
                    s.phase = kPhaseDone;
                    continue;
                }
                if (hr_cmp_pos(dzdcNormTrue, zero) > 0) {
                    const hreal<F> lhsTight = hr_reduced(hr_mul(zNorm, s.sqr_scale));
                    if (hr_cmp_pos(lhsTight, rhs) < 0) {
                        const hreal<F> newSqr = hr_reduced(hr_div(lhsTight, dzdcNormTrue));
                        if (hr_cmp_pos(newSqr, zero) > 0)
                            s.sqr_r = newSqr;
                    }
                }
                if (s.step >= s.cap) {
                    s.phase = kPhaseDone;
                    out[i] = typename FsFeatRec<F>::Out{};
                }
            } else if (s.step >= s.cap) {
                // fixed-period path, :1932-1942
                store_out<F>(out[i], FS_FEATURE_OK, (uint64_t)(IterT)s.period, hc_reduced(s.z),
                             hc_reduced(hc_mul(s.dzdc, invScaleC)), hc_reduced(hc_mul(s.zcoeff, invScaleC)),
                             hr_reduced(hc_norm2(s.z)));
                s.phase = kPhaseDone;
            }
        } else if (s.phase == kPhaseDirect) {
            direct_fixed_trip<F, IterT>(s, out[i], one, two, escape2, oneC);
        }
    }
    return s;
}

// the lanes of this wave that are still running, added to *unfinished
__device__ __forceinline__ void count_unfinished(uint32_t phase, uint32_t *unfinished)
{
    const uint64_t left = __ballot(phase != kPhaseDone);
    if (threadIdx.x == 0 && left != 0)
        atomicAdd(unfinished, (uint32_t)__popcll(left));
}

// Up to `slice` steps of every unfinished candidate, on the expanded orbit.
template <class F, class IterT>
__global__ void __launch_bounds__(64) k_feature_step(const typename FsDev<F>::Z *__restrict__ zref, uint32_t count,
                                                      FsFeatLane<F> *__restrict__ st,
                                                      typename FsFeatRec<F>::Out *__restrict__ out, uint64_t n, int find,
                                                      uint32_t slice, uint32_t *__restrict__ unfinished)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    FsFeatLane<F> s;
    if (i < n)
        s = st[i];
    else
        s.phase = kPhaseDone;
    ExpandedOrbit<F> orbit{zref, count, s.ref};
    s = feature_slice<F, IterT>(s, orbit, out, i, find, slice);
    s.ref = orbit.ref;
    if (i < n)
        st[i] = s;
    count_unfinished(s.phase, unfinished);
}

// ... on the waypoint-resident orbit.  Positions (the lane's, the waypoints' indices, count) are IterT-wide.
template <class F, class IterT>
__global__ void __launch_bounds__(64) k_feature_step_seq(const typename FsWaypoints<F>::Rec *__restrict__ wp, uint32_t n_wp,
                                                          hreal<F> cx, hreal<F> cy, IterT count,
                                                          FsFeatSeqLane<F, IterT> *__restrict__ st,
                                                          typename FsFeatRec<F>::Out *__restrict__ out, uint64_t n, int find,
                                                          uint32_t slice, uint32_t *__restrict__ unfinished)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    FsFeatSeqLane<F, IterT> s;
    if (i < n)
        s = st[i];
    else
        s.phase = kPhaseDone;
    WaypointOrbit<F, IterT> orbit;
    orbit.count = count;
    orbit.seq.wp = wp, orbit.seq.n_wp = n_wp;
    orbit.seq.cx = cx, orbit.seq.cy = cy;
    orbit.seq.idx = s.ref, orbit.seq.next = s.next, orbit.seq.next_index = s.next_index;
    orbit.seq.zx = s.zx, orbit.seq.zy = s.zy;
    s = feature_slice<F, IterT>(s, orbit, out, i, find, slice);
    if (i < n) {
        s.ref = orbit.seq.idx, s.next = orbit.seq.next, s.next_index = orbit.seq.next_index;
        s.zx = orbit.seq.zx, s.zy = orbit.seq.zy;
        st[i] = s;
    }
    count_unfinished(s.phase, unfinished);
}

} // namespace

template <class F>
void fsk_feature_init(const void *in, FsFeatLane<F> *st, void *out, uint64_t n, int find, hreal<F> R, uint64_t max_iters,
                      uint64_t count, hipStream_t s)
{
    hipLaunchKernelGGL((k_feature_init<F, FsFeatLane<F>, NoCursor>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s,
                       (const typename FsFeatRec<F>::In *)in, st, (typename FsFeatRec<F>::Out *)out, n, find, R, max_iters,
                       count, NoCursor{});
}

template <class F> size_t fsk_feature_seq_lane_bytes(int iter_u64)
{
    return iter_u64 ? sizeof(FsFeatSeqLane<F, uint64_t>) : sizeof(FsFeatSeqLane<F, uint32_t>);
}

template <class F>
void fsk_feature_seq_init(const void *in, void *st, void *out, uint64_t n, int find, hreal<F> R, uint64_t max_iters,
                          uint64_t count, const void *wp, uint32_t n_wp, int iter_u64, hipStream_t s)
{
    auto launch = [&](auto pos) {
        using PosT = decltype(pos);
        const CursorAtStart<F, PosT> start{(const typename FsWaypoints<F>::Rec *)wp, n_wp};
        hipLaunchKernelGGL((k_feature_init<F, FsFeatSeqLane<F, PosT>, CursorAtStart<F, PosT>>), dim3((unsigned)((n + 63) / 64)),
                           dim3(64), 0, s, (const typename FsFeatRec<F>::In *)in, (FsFeatSeqLane<F, PosT> *)st,
                           (typename FsFeatRec<F>::Out *)out, n, find, R, max_iters, count, start);
    };
    if (iter_u64)
        launch(uint64_t(0));
    else
        launch(uint32_t(0));
}

template <class F>
void fsk_feature_seq_step(const void *wp, uint32_t n_wp, const typename FsDev<F>::Real *c_low, uint64_t count, void *st,
                          void *out, uint64_t n, int find, int iter_u64, uint32_t slice, uint32_t *unfinished, hipStream_t s)
{
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    auto *o = (typename FsFeatRec<F>::Out *)out;
    const auto *w = (const typename FsWaypoints<F>::Rec *)wp;
    const hreal<F> cx{c_low[0].m, c_low[0].e}, cy{c_low[1].m, c_low[1].e};
    if (iter_u64)
        hipLaunchKernelGGL((k_feature_step_seq<F, uint64_t>), grid, block, 0, s, w, n_wp, cx, cy, count,
                           (FsFeatSeqLane<F, uint64_t> *)st, o, n, find, slice, unfinished);
    else
        hipLaunchKernelGGL((k_feature_step_seq<F, uint32_t>), grid, block, 0, s, w, n_wp, cx, cy, (uint32_t)count,
                           (FsFeatSeqLane<F, uint32_t> *)st, o, n, find, slice, unfinished);
}

template <class F>
void fsk_feature_step(const typename FsDev<F>::Z *zref, uint32_t count, FsFeatLane<F> *st, void *out, uint64_t n, int find,
                      int iter_u64, uint32_t slice, uint32_t *unfinished, hipStream_t s)
{
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    auto *o = (typename FsFeatRec<F>::Out *)out;
    if (iter_u64)
        hipLaunchKernelGGL((k_feature_step<F, uint64_t>), grid, block, 0, s, zref, count, st, o, n, find, slice, unfinished);
    else
        hipLaunchKernelGGL((k_feature_step<F, uint32_t>), grid, block, 0, s, zref, count, st, o, n, find, slice, unfinished);
}

template void fsk_feature_init<float>(const void *, FsFeatLane<float> *, void *, uint64_t, int, hreal<float>, uint64_t,
                                      uint64_t, hipStream_t);
template void fsk_feature_init<double>(const void *, FsFeatLane<double> *, void *, uint64_t, int, hreal<double>, uint64_t,
                                       uint64_t, hipStream_t);
template void fsk_feature_step<float>(const float4 *, uint32_t, FsFeatLane<float> *, void *, uint64_t, int, int, uint32_t,
                                      uint32_t *, hipStream_t);
template void fsk_feature_step<double>(const FsZ64 *, uint32_t, FsFeatLane<double> *, void *, uint64_t, int, int, uint32_t,
                                       uint32_t *, hipStream_t);
template size_t fsk_feature_seq_lane_bytes<float>(int);
template size_t fsk_feature_seq_lane_bytes<double>(int);
template void fsk_feature_seq_init<float>(const void *, void *, void *, uint64_t, int, hreal<float>, uint64_t, uint64_t,
                                          const void *, uint32_t, int, hipStream_t);
template void fsk_feature_seq_init<double>(const void *, void *, void *, uint64_t, int, hreal<double>, uint64_t, uint64_t,
                                           const void *, uint32_t, int, hipStream_t);
template void fsk_feature_seq_step<float>(const void *, uint32_t, const fs_real_hdr32 *, uint64_t, void *, void *, uint64_t, int,
                                          int, uint32_t, uint32_t *, hipStream_t);
template void fsk_feature_seq_step<double>(const void *, uint32_t, const fs_real_hdr64 *, uint64_t, void *, void *, uint64_t, int,
                                           int, uint32_t, uint32_t *, hipStream_t);
