// kernels_feature_direct.hip -- the Feature Finder's Direct evaluator (fs_feature_eval_direct): one lane per candidate, no
// reference orbit.
//
// Restates, operation for operation, in the arithmetic of hdr_math.hpp (HDRFloat<float | double>):
//   FeatureFinder::Evaluate_FindPeriod_Direct               FeatureFinder.cpp:1576-1660
//   FeatureFinder::Evaluate_PeriodResidualAndDzdc_Direct    FeatureFinder.cpp:1661-1711   (feature_steps.hpp, shared with PT)
//   DirectEvaluator::Eval (find => the first, fixed => the second, no fallback)  FeatureFinder.cpp:2188-2211
// Points the reference fixes and this file keeps: zcoeff and dzdc are advanced with the previous step's z; the period search adds
// a fresh, unreduced C(one, T{}) to dzdc each step where the fixed-period loop adds its reduced oneC; an escape (|z|^2 > 4096)
// ends the search as rejected, before the trigger is looked at; the trigger is |z|^2 < R^2 |dzdc|^2 with the R^2 of the call,
// never tightened; a trigger at a step IterType cannot hold rejects; R <= 0 rejects.
//
// The evaluation runs in bounded slices like fs_feature_eval, the lane state kept in FsFeatDirectLane records between launches.
// The lanes of a wave finish at very different steps (escapers in tens, triggers in hundreds to thousands): a finished lane only
// idles in its slot, and a wave leaves the slice loop as soon as a ballot finds none of its lanes running.  All candidates of a
// call are in the same mode, so the two loop bodies never share a wave.
#include "feature_steps.hpp"

using namespace fs;
using namespace fsfeat;

namespace {

template <class F>
__global__ void __launch_bounds__(64) k_feature_direct_init(const typename FsFeatRec<F>::In *__restrict__ in,
                                                             FsFeatDirectLane<F> *__restrict__ st,
                                                             typename FsFeatRec<F>::Out *__restrict__ out, uint64_t n, int find,
                                                             hreal<F> R, uint64_t max_iters)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const auto inp = in[i];
    FsFeatDirectLane<F> s;
    s.c = hcplx<F>{inp.c.re, inp.c.im, inp.c.e};
    s.z = hc_zero<F>();
    s.dzdc = hc_zero<F>();
    s.zcoeff = hc_zero<F>();
    s.step = 0;
    s.period = inp.period;
    s.cap = find ? max_iters : inp.period;
    s.phase = find ? kPhaseFindDirect : kPhaseDirect;
    s.pad_ = 0;
    if (find) {
        // :1588-1593, and a loop of no trips (:1608) falls through to `return false`
        hr_reduce(R);
        if (hr_cmp_pos(R, hr_zero<F>()) <= 0 || s.cap < 1) {
            s.phase = kPhaseDone;
            out[i] = typename FsFeatRec<F>::Out{};
        }
    }
    st[i] = s;
}

template <class F, class IterT>
__global__ void __launch_bounds__(64) k_feature_direct_step(FsFeatDirectLane<F> *__restrict__ st,
                                                             typename FsFeatRec<F>::Out *__restrict__ out, uint64_t n, int find,
                                                             hreal<F> R, uint32_t slice, uint32_t *__restrict__ unfinished)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    FsFeatDirectLane<F> s;
    if (i < n)
        s = st[i];
    else
        s.phase = kPhaseDone;
    if (__ballot(s.phase != kPhaseDone) == 0)
        return; // every lane of the wave finished in an earlier slice: nothing to load further, nothing to write back

    const hreal<F> zero = hr_zero<F>();
    const hreal<F> one = hr_from_number<F>(F(1));
    const hreal<F> two = hr_from_number<F>(F(2));
    const hreal<F> escape2 = hr_from_number<F>(F(4096));

    if (find) {
        hr_reduce(R);
        const hreal<F> R2 = hr_reduced(hr_mul(R, R));
        const hcplx<F> oneFresh = hc_from_hr(one, zero); // C(one, T{}), :1619
        for (uint32_t k = 0; k < slice; ++k) {
            if (__ballot(s.phase != kPhaseDone) == 0)
                break;
            if (s.phase != kPhaseDone) {
                // Evaluate_FindPeriod_Direct loop body, :1608-1657
                if (s.step == 0)
                    s.zcoeff = hc_from_hr(one, zero);
                else
                    s.zcoeff = hc_mul(s.zcoeff, hc_mul_real(s.z, two));
                hc_reduce(s.zcoeff);
                s.dzdc = hc_add(hc_mul(s.dzdc, hc_mul_real(s.z, two)), oneFresh);
                hc_reduce(s.dzdc);
                s.z = hc_add(hc_mul(s.z, s.z), s.c);
                hc_reduce(s.z);
                s.step++;

                const hreal<F> z2 = hr_reduced(hc_norm2(s.z));
                if (hr_cmp_pos(z2, escape2) > 0) {
                    s.phase = kPhaseDone;
                    out[i] = typename FsFeatRec<F>::Out{};
                    continue;
                }
                const hreal<F> d2 = hr_reduced(hc_norm2(s.dzdc));
                const hreal<F> rhs = hr_reduced(hr_mul(R2, d2));
                if (hr_cmp_pos(z2, rhs) < 0) {
                    // cand = n + 1 must fit IterType (:1643-1655)
                    if (s.step <= (uint64_t)(IterT)~(IterT)0)
                        store_out<F>(out[i], FS_FEATURE_OK_DIRECT, (uint64_t)(IterT)s.step, s.z, s.dzdc, s.zcoeff, z2);
                    else
                        out[i] = typename FsFeatRec<F>::Out{};
                    s.phase = kPhaseDone;
                } else if (s.step >= s.cap) {
                    s.phase = kPhaseDone;
                    out[i] = typename FsFeatRec<F>::Out{};
                }
            }
        }
    } else {
        const hcplx<F> oneC = hc_reduced(hc_from_hr(one, zero));
        for (uint32_t k = 0; k < slice; ++k) {
            if (__ballot(s.phase != kPhaseDone) == 0)
                break;
            if (s.phase != kPhaseDone)
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
void fsk_feature_direct_init(const void *in, FsFeatDirectLane<F> *st, void *out, uint64_t n, int find, hreal<F> R,
                             uint64_t max_iters, hipStream_t s)
{
    hipLaunchKernelGGL(k_feature_direct_init<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s,
                       (const typename FsFeatRec<F>::In *)in, st, (typename FsFeatRec<F>::Out *)out, n, find, R, max_iters);
}

template <class F>
void fsk_feature_direct_step(FsFeatDirectLane<F> *st, void *out, uint64_t n, int find, int iter_u64, hreal<F> R, uint32_t slice,
                             uint32_t *unfinished, hipStream_t s)
{
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    auto *o = (typename FsFeatRec<F>::Out *)out;
    if (iter_u64)
        hipLaunchKernelGGL((k_feature_direct_step<F, uint64_t>), grid, block, 0, s, st, o, n, find, R, slice, unfinished);
    else
        hipLaunchKernelGGL((k_feature_direct_step<F, uint32_t>), grid, block, 0, s, st, o, n, find, R, slice, unfinished);
}

template void fsk_feature_direct_init<float>(const void *, FsFeatDirectLane<float> *, void *, uint64_t, int, hreal<float>,
                                             uint64_t, hipStream_t);
template void fsk_feature_direct_init<double>(const void *, FsFeatDirectLane<double> *, void *, uint64_t, int, hreal<double>,
                                              uint64_t, hipStream_t);
template void fsk_feature_direct_step<float>(FsFeatDirectLane<float> *, void *, uint64_t, int, int, hreal<float>, uint32_t,
                                             uint32_t *, hipStream_t);
template void fsk_feature_direct_step<double>(FsFeatDirectLane<double> *, void *, uint64_t, int, int, hreal<double>, uint32_t,
                                              uint32_t *, hipStream_t);
