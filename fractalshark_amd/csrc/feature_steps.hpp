// feature_steps.hpp -- device pieces shared by the Feature Finder's two evaluators: kernels_feature.hip (fs_feature_eval, PT with
// the Direct fallback) and kernels_feature_direct.hip (fs_feature_eval_direct).  The fixed-period Direct loop exists once, here.
#pragma once
#include "kernels.h"
#include "../../include/fsmi355.h"

namespace fsfeat {

using namespace fs;

// A lane's phase.  kPhasePT / kPhaseDirect / kPhaseDone are the states of FsFeatLane (kernels.h); kPhaseFindDirect is the
// period search of FsFeatDirectLane.
enum : uint32_t { kPhasePT = 0, kPhaseDirect = 1, kPhaseDone = 2, kPhaseFindDirect = 3 };

__device__ __forceinline__ fs_cplx_hdr32 rec(hcplx32 a) { return fs_cplx_hdr32{a.re, a.im, a.e}; }
__device__ __forceinline__ fs_cplx_hdr64 rec(hcplx64 a) { return fs_cplx_hdr64{a.re, a.im, a.e, 0}; }
__device__ __forceinline__ fs_real_hdr32 rec(hreal32 a) { return fs_real_hdr32{a.m, a.e}; }
__device__ __forceinline__ fs_real_hdr64 rec(hreal64 a) { return fs_real_hdr64{a.m, a.e, 0}; }

template <class F>
__device__ __forceinline__ void store_out(typename FsFeatRec<F>::Out &o, uint32_t status, uint64_t period, hcplx<F> diff,
                                          hcplx<F> dzdc, hcplx<F> zcoeff, hreal<F> residual2)
{
    typename FsFeatRec<F>::Out r{};
    r.status = status;
    r.period = period;
    r.diff = rec(diff);
    r.dzdc = rec(dzdc);
    r.zcoeff = rec(zcoeff);
    r.residual2 = rec(residual2);
    o = r;
}

// One trip of Evaluate_PeriodResidualAndDzdc_Direct, FeatureFinder.cpp:1677-1710 (period steps counted at IterType width), for a
// lane in kPhaseDirect: Lane = FsFeatLane<F> or FsFeatDirectLane<F> (step, cap, period, z, dzdc, zcoeff, c, phase).  oneC is
// the reduced C(one, T{}) of :1673-1676.
template <class F, class IterT, class Lane>
__device__ __forceinline__ void direct_fixed_trip(Lane &s, typename FsFeatRec<F>::Out &o, hreal<F> one, hreal<F> two,
                                                  hreal<F> escape2, hcplx<F> oneC)
{
    if ((IterT)s.step >= (IterT)s.cap) {
        store_out<F>(o, FS_FEATURE_OK_DIRECT, (uint64_t)(IterT)s.period, s.z, s.dzdc, s.zcoeff, hr_reduced(hc_norm2(s.z)));
        s.phase = kPhaseDone;
        return;
    }
    if (s.step == 0)
        s.zcoeff = hc_from_hr(one, hr_zero<F>());
    else
        s.zcoeff = hc_mul(s.zcoeff, hc_mul_real(s.z, two));
    hc_reduce(s.zcoeff);
    s.dzdc = hc_add(hc_mul(s.dzdc, hc_mul_real(s.z, two)), oneC);
    hc_reduce(s.dzdc);
    s.z = hc_add(hc_mul(s.z, s.z), s.c);
    hc_reduce(s.z);
    s.step++;
    if (hr_cmp_pos(hr_reduced(hc_norm2(s.z)), escape2) > 0) {
        s.phase = kPhaseDone;
        o = typename FsFeatRec<F>::Out{};
    }
}

} // namespace fsfeat
