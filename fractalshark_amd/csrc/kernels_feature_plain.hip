// kernels_feature_plain.hip -- the Feature Finder's evaluators for T = float / double (fs_feature_eval_plain,
// fs_feature_eval_plain_direct): one lane per candidate.  What the reference runs for the algorithms whose MainType is a plain
// type (FeatureFinderOrchestrator.cpp:457-469, FeatureFinder.cpp:2740-2795) -- Gpu1x32PerturbedLAv2*, its automatic choice for
// every zoom factor below 1e34 (Fractal.cpp:961-971), among them.
//
// Restates, operation for operation, in IEEE binary32 / binary64 with C = FloatComplex<T> (FloatComplex.h: plus_mutable :174-179,
// times_mutable :182-194 and :224-229, norm_squared :302-305; Reduce is empty, :290-292):
//   FeatureFinder::Evaluate_PT<true | false>                 FeatureFinder.cpp:1757-1921
//   PeriodicityPP::Init / CheckPeriodicity                   FeatureFinder.cpp:1471-1534
//   FeatureFinder::Evaluate_FindPeriod_Direct                FeatureFinder.cpp:1576-1660
//   FeatureFinder::Evaluate_PeriodResidualAndDzdc_Direct     FeatureFinder.cpp:1661-1711
//   PTEvaluator::Eval (PT, then Direct when a fixed-period PT evaluation escapes)  :2313-2354;  DirectEvaluator::Eval  :2188-2211
// Compiled with -ffp-contract=off: every operation below is one IEEE operation as written -- no fused multiply-add, `/` is the
// correctly rounded division, subnormals are kept (gfx950's default mode; see the head of hdr_math.hpp).  Compares are the plain
// operators (HDRFloat.h:1536-1586), so a NaN compares false everywhere, as it does in the reference.
//
// Points the reference fixes and this file keeps: escape radius^2 4096; the rebase test (refIteration >= count - 1 or
// |z|^2 < |dz|^2) comes before the escape test; zcoeff and dzdc are advanced with the previous step's z; count >= 2, cap >= 1
// and R > 0 are set-up rejects.  The unit scaling factor (scaleExp = 0: ScalingFactor = InvScalingFactor = ldexp(1, 0) = 1):
//   dzdc + ScalingFactorC and zcoeff = ScalingFactorC     are the additions / the assignment of (1, 0) themselves;
//   |dzdc|^2 * InvScale2                                  is performed (x * 1 returns x bit for bit for every x, NaNs included,
//                                                          so the compiler may fold it: no bit can change);
//   dzdc * InvScalingFactorC, zcoeff * InvScalingFactorC  are performed in full, (re 1 - im 0, re 0 + im 1): NOT the identity --
//                                                          a zero component can change sign (-0 - (-0) = +0) and an infinite
//                                                          one makes a NaN (inf * 0) -- so they cannot be dropped; they run
//                                                          once per accepted candidate, outside the step.
//
// The shape of kernels_feature.hip: 64-lane workgroups, bounded slices with the lane state in device memory between launches
// (FsFeatPLane / FsFeatPSeqLane / FsFeatPDirectLane, feature_plain.hpp), a ballot ends a wave's loop when none of its lanes runs,
// the count of unfinished lanes comes back after every slice.  While a wave's PT lanes agree on the orbit position the step's
// two entries are read once for the wave through the constant address space, else each lane loads its own.  On a
// waypoint-resident orbit every lane carries a decompression cursor, the plain-type twin of SeqOrbit (seq_orbit.hpp) with the
// operations of SeqPlain (kernels_plain.hip) and positions as wide as the IterType.
#include "feature_plain.hpp"
#include "feature_steps.hpp"

using namespace fsfeat; // the phases

namespace {

template <class T> using PC = FsPC<T>;

template <class T> __device__ __forceinline__ PC<T> operator+(PC<T> a, PC<T> b) { return PC<T>{a.re + b.re, a.im + b.im}; }
// times_mutable(FloatComplex)
template <class T> __device__ __forceinline__ PC<T> operator*(PC<T> a, PC<T> b)
{
    const T re = (a.re * b.re) - (a.im * b.im);
    const T im = (a.re * b.im) + (a.im * b.re);
    return PC<T>{re, im};
}
// times_mutable(SubType)
template <class T> __device__ __forceinline__ PC<T> mul_real(PC<T> a, T f) { return PC<T>{a.re * f, a.im * f}; }
template <class T> __device__ __forceinline__ T norm2(PC<T> a) { return a.re * a.re + a.im * a.im; }

template <class T>
__device__ __forceinline__ void store_plain(typename FsFeatPRec<T>::Out &o, uint32_t status, uint64_t period, PC<T> diff,
                                          PC<T> dzdc, PC<T> zcoeff, T residual2)
{
    typename FsFeatPRec<T>::Out r{};
    r.status = status;
    r.period = period;
    r.diff[0] = diff.re, r.diff[1] = diff.im;
    r.dzdc[0] = dzdc.re, r.dzdc[1] = dzdc.im;
    r.zcoeff[0] = zcoeff.re, r.zcoeff[1] = zcoeff.im;
    r.residual2 = residual2;
    o = r;
}

// The waypoint cursor for a plain T with PosT-wide positions: SeqOrbit's state and interface, SeqPlain's arithmetic
// (runOneIter, PerturbationResultsHelpers.h:51-58: the operations, in the order, of k_decompress_plain, which expands the same
// waypoints once per upload -- both forms see the same orbit bit for bit).
template <class T, class PosT> struct PlainCursor {
    const typename FsFeatPRec<T>::Waypoint *__restrict__ wp;
    uint32_t n_wp;
    T cx, cy;
    PosT idx;        // orbit index of (zx, zy)
    uint32_t next;   // number of the first waypoint behind the cursor
    PosT next_index; // ... and its orbit index (all ones: none left)
    T zx, zy;

    __device__ __forceinline__ PosT index_of(uint32_t k) const { return (PosT)(wp[k].index_and_rebase & 0x7FFFFFFFFFFFFFFFull); }
    __device__ __forceinline__ void step()
    {
        idx++;
        if (idx == next_index) {
            zx = wp[next].x, zy = wp[next].y;
            next++;
            next_index = next < n_wp ? index_of(next) : ~(PosT)0;
        } else {
            const T zx_old = zx;
            zx = zx * zx - zy * zy + cx;
            zy = T(2.0f) * zx_old * zy + cy;
        }
    }
    // waypoint 0 sits at index 0
    __device__ __forceinline__ void rewind()
    {
        zx = wp[0].x, zy = wp[0].y;
        idx = 0;
        next = 1u;
        next_index = next < n_wp ? index_of(next) : ~(PosT)0;
    }
};

// How the two orbit entries of a step arrive (the interface of kernels_feature.hip's): pair() yields the entries at the position
// and behind it and moves the position on by one, at_end() is the reference's refIteration >= count - 1, rebase() goes back to 0.
// A PT lane's position is at most count - 2 when pair() is called (count >= 2 is a set-up reject, and a lane that arrives at
// count - 1 rebases in the same step), so the reads stay inside the count entries and the cursor never steps past the last one.
template <class T> struct ExpandedPlain {
    using E = typename FsFeatPRec<T>::Orbit;
    const E *__restrict__ zref;
    uint32_t count;
    uint32_t ref;

    __device__ __forceinline__ void pair(PC<T> &zr, PC<T> &zr1)
    {
        typedef const __attribute__((address_space(4))) E *EC;
        // once for the wave when its PT lanes agree on the position
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)ref);
        if (__builtin_amdgcn_ballot_w64(ref == first) == __builtin_amdgcn_ballot_w64(true)) {
            const EC zc = (EC)(uintptr_t)zref;
            zr = PC<T>{zc[first].x, zc[first].y};
            zr1 = PC<T>{zc[first + 1].x, zc[first + 1].y};
        } else {
            zr = PC<T>{zref[ref].x, zref[ref].y};
            zr1 = PC<T>{zref[ref + 1].x, zref[ref + 1].y};
        }
        ref++;
    }
    __device__ __forceinline__ bool at_end() const { return ref >= count - 1; }
    __device__ __forceinline__ void rebase() { ref = 0; }
};

template <class T, class PosT> struct WaypointPlain {
    PlainCursor<T, PosT> seq;
    PosT count;

    __device__ __forceinline__ void pair(PC<T> &zr, PC<T> &zr1)
    {
        zr = PC<T>{seq.zx, seq.zy};
        seq.step();
        zr1 = PC<T>{seq.zx, seq.zy};
    }
    __device__ __forceinline__ bool at_end() const { return seq.idx >= count - 1; }
    __device__ __forceinline__ void rebase() { seq.rewind(); }
};

// One trip of Evaluate_PeriodResidualAndDzdc_Direct (:1678-1710, period steps counted at IterType width) for a lane in
// kPhaseDirect.  oneC.Reduce() is empty: the loop adds (1, 0).
template <class T, class IterT, class Lane>
__device__ __forceinline__ void direct_fixed_trip_plain(Lane &s, typename FsFeatPRec<T>::Out &o)
{
    if ((IterT)s.step >= (IterT)s.cap) {
        store_plain<T>(o, FS_FEATURE_OK_DIRECT, (uint64_t)(IterT)s.period, s.z, s.dzdc, s.zcoeff, norm2(s.z));
        s.phase = kPhaseDone;
        return;
    }
    const PC<T> oneC{T(1.0), T(0)};
    if (s.step == 0)
        s.zcoeff = oneC;
    else
        s.zcoeff = s.zcoeff * mul_real(s.z, T(2.0));
    s.dzdc = s.dzdc * mul_real(s.z, T(2.0)) + oneC;
    s.z = (s.z * s.z) + s.c;
    s.step++;
    if (norm2(s.z) > T(4096.0)) {
        s.phase = kPhaseDone;
        o = typename FsFeatPRec<T>::Out{};
    }
}

// Evaluate_PT's set-up (:1773-1824) and PeriodicityPP::Init (:1478-1494); a candidate that fails it is finished here (rejected in
// find mode, handed to the Direct loop in fixed mode, as PTEvaluator::Eval does).  Lane = FsFeatPLane<T> or
// FsFeatPSeqLane<T, PosT>, whose cursor starts at waypoint 0.
template <class T, class Lane, bool kSeq>
__global__ void __launch_bounds__(64) k_featp_init(const typename FsFeatPRec<T>::In *__restrict__ in, Lane *__restrict__ st,
                                                    typename FsFeatPRec<T>::Out *__restrict__ out, uint64_t n, int find, T R,
                                                    uint64_t max_iters, uint64_t count,
                                                    const typename FsFeatPRec<T>::Waypoint *__restrict__ wp, uint32_t n_wp)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const auto inp = in[i];
    Lane s;
    s.dc = PC<T>{inp.dc[0], inp.dc[1]};
    s.c = PC<T>{inp.c[0], inp.c[1]};
    s.period = inp.period;
    s.z = s.dz = s.dzdc = s.zcoeff = PC<T>{T(0), T(0)};
    s.sqr_r = T(0);
    s.step = 0;
    s.ref = 0;
    s.cap = find ? max_iters : inp.period;
    s.phase = kPhasePT;
    if constexpr (kSeq) {
        s.zx = wp[0].x, s.zy = wp[0].y;
        s.next = 1u;
        s.next_index = 1u < n_wp ? (decltype(s.next_index))(wp[1].index_and_rebase & 0x7FFFFFFFFFFFFFFFull)
                                 : ~(decltype(s.next_index))0;
    }
    bool ok = count >= 2 && s.cap >= 1;
    if (ok && find) {
        if (R <= T(0))
            ok = false;
        else
            s.sqr_r = R * R; // PeriodicityPP::Init; SqrNearLinearRadiusScale = 0.25 * 0.25, the constant of the step
    }
    if (!ok) {
        if (find) {
            s.phase = kPhaseDone;
            out[i] = typename FsFeatPRec<T>::Out{};
        } else {
            s.phase = kPhaseDirect;
            s.cap = inp.period;
        }
    }
    st[i] = s;
}

// Up to `slice` steps of one candidate (every lane of the wave calls it).  IterT = the reference's IterType: the width periods
// are counted at.  The orbit position is the Orbit's, not the lane's `ref`.
template <class T, class IterT, class Lane, class Orbit>
__device__ __forceinline__ Lane featp_slice(Lane s, Orbit &orbit, typename FsFeatPRec<T>::Out *out, uint64_t i, int find,
                                            uint32_t slice)
{
    const T zero = T(0), one = T(1.0), two = T(2.0), escape2 = T(4096.0);
    const T near1 = T(0.25);
    const T sqr_scale = near1 * near1;
    const PC<T> scaleC{one, zero}, invScaleC{one, zero}; // C(ScalingFactor, T{}), C(InvScalingFactor, T{})
    const T invScale2 = one * one;

    for (uint32_t k = 0; k < slice; ++k) {
        if (__ballot(s.phase != kPhaseDone) == 0)
            break;
        if (s.phase == kPhasePT) {
            // Evaluate_PT loop body, :1826-1896
            if (s.step == 0)
                s.zcoeff = scaleC;
            else
                s.zcoeff = s.zcoeff * mul_real(s.z, two);
            s.dzdc = s.dzdc * mul_real(s.z, two) + scaleC;

            // the orbit entries at refIteration and refIteration + 1; the position is refIteration + 1 afterwards
            PC<T> zr, zr1;
            orbit.pair(zr, zr1);

            s.dz = s.dz * (zr + s.z) + s.dc;
            s.z = zr1 + s.dz;

            const T dzNorm = norm2(s.dz);
            const T zNorm = norm2(s.z);
            if (orbit.at_end() || zNorm < dzNorm) {
                s.dz = s.z;
                orbit.rebase();
            }
            s.step++;

            if (zNorm > escape2) {
                if (find) {
                    s.phase = kPhaseDone;
                    out[i] = typename FsFeatPRec<T>::Out{};
                } else {
                    // PTEvaluator::Eval<false>: PT failed, DIRECT at the same period
                    s.phase = kPhaseDirect;
                    s.cap = s.period;
                    s.step = 0;
                    s.z = s.dzdc = s.zcoeff = PC<T>{zero, zero};
                }
                continue;
            }

            if (find) {
                const T dzdcNormTrue = norm2(s.dzdc) * invScale2;
                // PeriodicityPP::CheckPeriodicity
                const T rhs = s.sqr_r * dzdcNormTrue;
                if (zNorm < rhs) {
                    store_plain<T>(out[i], FS_FEATURE_OK, (uint64_t)(IterT)s.step, s.z, s.dzdc * invScaleC, s.zcoeff * invScaleC,
                                 zNorm);
                    s.phase = kPhaseDone;
                    continue;
                }
                if (dzdcNormTrue > zero) {
                    const T lhsTight = zNorm * sqr_scale;
                    if (lhsTight < rhs) {
                        const T newSqr = lhsTight / dzdcNormTrue;
                        if (newSqr > zero)
                            s.sqr_r = newSqr;
                    }
                }
                if (s.step >= s.cap) {
                    s.phase = kPhaseDone;
                    out[i] = typename FsFeatPRec<T>::Out{};
                }
            } else if (s.step >= s.cap) {
                // fixed-period path, :1907-1917
                store_plain<T>(out[i], FS_FEATURE_OK, (uint64_t)(IterT)s.period, s.z, s.dzdc * invScaleC, s.zcoeff * invScaleC,
                             norm2(s.z));
                s.phase = kPhaseDone;
            }
        } else if (s.phase == kPhaseDirect) {
            direct_fixed_trip_plain<T, IterT>(s, out[i]);
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
template <class T, class IterT>
__global__ void __launch_bounds__(64) k_featp_step(const typename FsFeatPRec<T>::Orbit *__restrict__ zref, uint32_t count,
                                                    FsFeatPLane<T> *__restrict__ st,
                                                    typename FsFeatPRec<T>::Out *__restrict__ out, uint64_t n, int find,
                                                    uint32_t slice, uint32_t *__restrict__ unfinished)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    FsFeatPLane<T> s;
    if (i < n)
        s = st[i];
    else
        s.phase = kPhaseDone;
    ExpandedPlain<T> orbit{zref, count, s.ref};
    s = featp_slice<T, IterT>(s, orbit, out, i, find, slice);
    s.ref = orbit.ref;
    if (i < n)
        st[i] = s;
    count_unfinished(s.phase, unfinished);
}

// ... on the waypoint-resident orbit.  Positions (the lane's, the waypoints' indices, count) are IterT-wide.
template <class T, class IterT>
__global__ void __launch_bounds__(64) k_featp_step_seq(const typename FsFeatPRec<T>::Waypoint *__restrict__ wp, uint32_t n_wp,
                                                        T cx, T cy, IterT count, FsFeatPSeqLane<T, IterT> *__restrict__ st,
                                                        typename FsFeatPRec<T>::Out *__restrict__ out, uint64_t n, int find,
                                                        uint32_t slice, uint32_t *__restrict__ unfinished)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    FsFeatPSeqLane<T, IterT> s;
    if (i < n)
        s = st[i];
    else
        s.phase = kPhaseDone;
    WaypointPlain<T, IterT> orbit;
    orbit.count = count;
    orbit.seq.wp = wp, orbit.seq.n_wp = n_wp;
    orbit.seq.cx = cx, orbit.seq.cy = cy;
    orbit.seq.idx = s.ref, orbit.seq.next = s.next, orbit.seq.next_index = s.next_index;
    orbit.seq.zx = s.zx, orbit.seq.zy = s.zy;
    s = featp_slice<T, IterT>(s, orbit, out, i, find, slice);
    if (i < n) {
        s.ref = orbit.seq.idx, s.next = orbit.seq.next, s.next_index = orbit.seq.next_index;
        s.zx = orbit.seq.zx, s.zy = orbit.seq.zy;
        st[i] = s;
    }
    count_unfinished(s.phase, unfinished);
}

// ---- Direct: no orbit.  Evaluate_FindPeriod_Direct's set-up (:1588-1593), and a loop of no trips (:1608) falls through to
// `return false`.
template <class T>
__global__ void __launch_bounds__(64) k_featp_direct_init(const typename FsFeatPRec<T>::In *__restrict__ in,
                                                           FsFeatPDirectLane<T> *__restrict__ st,
                                                           typename FsFeatPRec<T>::Out *__restrict__ out, uint64_t n, int find,
                                                           T R, uint64_t max_iters)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const auto inp = in[i];
    FsFeatPDirectLane<T> s;
    s.c = PC<T>{inp.c[0], inp.c[1]};
    s.z = s.dzdc = s.zcoeff = PC<T>{T(0), T(0)};
    s.step = 0;
    s.period = inp.period;
    s.cap = find ? max_iters : inp.period;
    s.phase = find ? kPhaseFindDirect : kPhaseDirect;
    s.pad_ = 0;
    if (find && (R <= T(0) || s.cap < 1)) {
        s.phase = kPhaseDone;
        out[i] = typename FsFeatPRec<T>::Out{};
    }
    st[i] = s;
}

// All candidates of a call are in the same mode, so the two loop bodies never share a wave.
template <class T, class IterT>
__global__ void __launch_bounds__(64) k_featp_direct_step(FsFeatPDirectLane<T> *__restrict__ st,
                                                           typename FsFeatPRec<T>::Out *__restrict__ out, uint64_t n, int find,
                                                           T R, uint32_t slice, uint32_t *__restrict__ unfinished)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    FsFeatPDirectLane<T> s;
    if (i < n)
        s = st[i];
    else
        s.phase = kPhaseDone;
    if (__ballot(s.phase != kPhaseDone) == 0)
        return; // every lane of the wave finished in an earlier slice: nothing to load further, nothing to write back

    if (find) {
        const T two = T(2.0), escape2 = T(4096.0);
        const T R2 = R * R;
        const PC<T> oneC{T(1.0), T(0)}; // C(one, T{}), :1619
        for (uint32_t k = 0; k < slice; ++k) {
            if (__ballot(s.phase != kPhaseDone) == 0)
                break;
            if (s.phase != kPhaseDone) {
                // Evaluate_FindPeriod_Direct loop body, :1608-1657
                if (s.step == 0)
                    s.zcoeff = oneC;
                else
                    s.zcoeff = s.zcoeff * mul_real(s.z, two);
                s.dzdc = s.dzdc * mul_real(s.z, two) + oneC;
                s.z = (s.z * s.z) + s.c;
                s.step++;

                const T z2 = norm2(s.z);
                if (z2 > escape2) {
                    s.phase = kPhaseDone;
                    out[i] = typename FsFeatPRec<T>::Out{};
                    continue;
                }
                const T d2 = norm2(s.dzdc);
                const T rhs = R2 * d2;
                if (z2 < rhs) {
                    // cand = n + 1 must fit IterType (:1643-1655)
                    if (s.step <= (uint64_t)(IterT)~(IterT)0)
                        store_plain<T>(out[i], FS_FEATURE_OK_DIRECT, (uint64_t)(IterT)s.step, s.z, s.dzdc, s.zcoeff, z2);
                    else
                        out[i] = typename FsFeatPRec<T>::Out{};
                    s.phase = kPhaseDone;
                } else if (s.step >= s.cap) {
                    s.phase = kPhaseDone;
                    out[i] = typename FsFeatPRec<T>::Out{};
                }
            }
        }
    } else {
        for (uint32_t k = 0; k < slice; ++k) {
            if (__ballot(s.phase != kPhaseDone) == 0)
                break;
            if (s.phase != kPhaseDone)
                direct_fixed_trip_plain<T, IterT>(s, out[i]);
        }
    }

    if (i < n)
        st[i] = s;
    count_unfinished(s.phase, unfinished);
}

} // namespace

template <class T> size_t fsk_featp_lane_bytes(int form, int iter_u64)
{
    if (form == kFeatPDirect)
        return sizeof(FsFeatPDirectLane<T>);
    if (form == kFeatPWaypoints)
        return iter_u64 ? sizeof(FsFeatPSeqLane<T, uint64_t>) : sizeof(FsFeatPSeqLane<T, uint32_t>);
    return sizeof(FsFeatPLane<T>);
}

template <class T>
void fsk_featp_init(int form, int iter_u64, const void *in, void *st, void *out, uint64_t n, int find, T R, uint64_t max_iters,
                    uint64_t count, const void *wp, uint32_t n_wp, hipStream_t s)
{
    using Rec = FsFeatPRec<T>;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    const auto *i = (const typename Rec::In *)in;
    auto *o = (typename Rec::Out *)out;
    const auto *w = (const typename Rec::Waypoint *)wp;
    if (form == kFeatPDirect)
        hipLaunchKernelGGL(k_featp_direct_init<T>, grid, block, 0, s, i, (FsFeatPDirectLane<T> *)st, o, n, find, R, max_iters);
    else if (form == kFeatPExpanded)
        hipLaunchKernelGGL((k_featp_init<T, FsFeatPLane<T>, false>), grid, block, 0, s, i, (FsFeatPLane<T> *)st, o, n, find, R,
                           max_iters, count, w, n_wp);
    else if (iter_u64)
        hipLaunchKernelGGL((k_featp_init<T, FsFeatPSeqLane<T, uint64_t>, true>), grid, block, 0, s, i,
                           (FsFeatPSeqLane<T, uint64_t> *)st, o, n, find, R, max_iters, count, w, n_wp);
    else
        hipLaunchKernelGGL((k_featp_init<T, FsFeatPSeqLane<T, uint32_t>, true>), grid, block, 0, s, i,
                           (FsFeatPSeqLane<T, uint32_t> *)st, o, n, find, R, max_iters, count, w, n_wp);
}

template <class T>
void fsk_featp_step(int form, int iter_u64, const void *orbit, uint32_t n_wp, T cx, T cy, uint64_t count, void *st, void *out,
                    uint64_t n, int find, T R, uint32_t slice, uint32_t *unfinished, hipStream_t s)
{
    using Rec = FsFeatPRec<T>;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    auto *o = (typename Rec::Out *)out;
    if (form == kFeatPDirect) {
        auto *d = (FsFeatPDirectLane<T> *)st;
        if (iter_u64)
            hipLaunchKernelGGL((k_featp_direct_step<T, uint64_t>), grid, block, 0, s, d, o, n, find, R, slice, unfinished);
        else
            hipLaunchKernelGGL((k_featp_direct_step<T, uint32_t>), grid, block, 0, s, d, o, n, find, R, slice, unfinished);
    } else if (form == kFeatPExpanded) {
        const auto *z = (const typename Rec::Orbit *)orbit;
        auto *l = (FsFeatPLane<T> *)st;
        if (iter_u64)
            hipLaunchKernelGGL((k_featp_step<T, uint64_t>), grid, block, 0, s, z, (uint32_t)count, l, o, n, find, slice, unfinished);
        else
            hipLaunchKernelGGL((k_featp_step<T, uint32_t>), grid, block, 0, s, z, (uint32_t)count, l, o, n, find, slice, unfinished);
    } else {
        const auto *w = (const typename Rec::Waypoint *)orbit;
        if (iter_u64)
            hipLaunchKernelGGL((k_featp_step_seq<T, uint64_t>), grid, block, 0, s, w, n_wp, cx, cy, count,
                               (FsFeatPSeqLane<T, uint64_t> *)st, o, n, find, slice, unfinished);
        else
            hipLaunchKernelGGL((k_featp_step_seq<T, uint32_t>), grid, block, 0, s, w, n_wp, cx, cy, (uint32_t)count,
                               (FsFeatPSeqLane<T, uint32_t> *)st, o, n, find, slice, unfinished);
    }
}

template size_t fsk_featp_lane_bytes<float>(int, int);
template size_t fsk_featp_lane_bytes<double>(int, int);
template void fsk_featp_init<float>(int, int, const void *, void *, void *, uint64_t, int, float, uint64_t, uint64_t, const void *,
                                    uint32_t, hipStream_t);
template void fsk_featp_init<double>(int, int, const void *, void *, void *, uint64_t, int, double, uint64_t, uint64_t,
                                     const void *, uint32_t, hipStream_t);
template void fsk_featp_step<float>(int, int, const void *, uint32_t, float, float, uint64_t, void *, void *, uint64_t, int, float,
                                    uint32_t, uint32_t *, hipStream_t);
template void fsk_featp_step<double>(int, int, const void *, uint32_t, double, double, uint64_t, void *, void *, uint64_t, int,
                                     double, uint32_t, uint32_t *, hipStream_t);
