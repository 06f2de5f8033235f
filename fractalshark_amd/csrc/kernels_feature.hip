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
#include "feature_steps.hpp"

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
template <class F>
__global__ void __launch_bounds__(64) k_feature_init(const typename FsFeatRec<F>::In *__restrict__ in,
                                                      FsFeatLane<F> *__restrict__ st, typename FsFeatRec<F>::Out *__restrict__ out,
                                                      uint64_t n, int find, hreal<F> R, uint64_t max_iters, uint64_t count)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const auto inp = in[i];
    FsFeatLane<F> s;
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

// Up to `slice` steps of every unfinished candidate.  IterT = the reference's IterType: the width periods are counted at.
template <class F, class IterT>
__global__ void __launch_bounds__(64) k_feature_step(const typename FsDev<F>::Z *__restrict__ zref, uint32_t count,
                                                      FsFeatLane<F> *__restrict__ st,
                                                      typename FsFeatRec<F>::Out *__restrict__ out, uint64_t n, int find,
                                                      uint32_t slice, uint32_t *__restrict__ unfinished)
{
    using Z = typename FsDev<F>::Z;
    typedef const __attribute__((address_space(4))) Z *ZC;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    FsFeatLane<F> s;
    if (i < n)
        s = st[i];
    else
        s.phase = kPhaseDone;

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

            // the orbit entries at refIteration and refIteration + 1: once for the wave when its PT lanes agree on the position
            hcplx<F> zr, zr1;
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.ref);
            if (__builtin_amdgcn_ballot_w64(s.ref == first) == __builtin_amdgcn_ballot_w64(true)) {
                // (through the constant address space: said explicitly, or the compiler folds the two arms into one vector load
                // of a per-lane selected index)
                const ZC zc = (ZC)(uintptr_t)zref;
                zr = OrbitRead<Z>::at(zc, first);
                zr1 = OrbitRead<Z>::at(zc, first + 1);
            } else {
                zr = OrbitRead<Z>::at(zref, s.ref);
                zr1 = OrbitRead<Z>::at(zref, s.ref + 1);
            }

            s.dz = hc_add(hc_mul(s.dz, hc_add(zr, s.z)), s.dc);
            hc_reduce(s.dz);
            s.ref++;
            s.z = hc_add(zr1, s.dz);
            hc_reduce(s.z);

            const hreal<F> dzNorm = hr_reduced(hc_norm2(s.dz));
            const hreal<F> zNorm = hr_reduced(hc_norm2(s.z));
            if (s.ref >= count - 1 || hr_cmp_pos(zNorm, dzNorm) < 0) {
                s.dz = hc_reduced(s.z);
                s.ref = 0;
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

    if (i < n)
        st[i] = s;
    const uint64_t left = __ballot(s.phase != kPhaseDone);
    if (threadIdx.x == 0 && left != 0)
        atomicAdd(unfinished, (uint32_t)__popcll(left));
}

} // namespace

template <class F>
void fsk_feature_init(const void *in, FsFeatLane<F> *st, void *out, uint64_t n, int find, hreal<F> R, uint64_t max_iters,
                      uint64_t count, hipStream_t s)
{
    hipLaunchKernelGGL(k_feature_init<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s,
                       (const typename FsFeatRec<F>::In *)in, st, (typename FsFeatRec<F>::Out *)out, n, find, R, max_iters,
                       count);
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
