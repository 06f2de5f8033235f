// tests/feature/feature_ref.cpp -- TEST INFRASTRUCTURE ONLY: CPU checker of the Feature Finder evaluator (fs_feature_eval).
//
// An independent restatement, on the oracle's pinned HDRFloat arithmetic (oracle/cpu_ref.cpp, included as it is), of
//   FeatureFinder::Evaluate_PT<true | false>                 FeatureFinder.cpp:1757-1958
//   PeriodicityPP::Init / CheckPeriodicity                   FeatureFinder.cpp:1471-1534
//   FeatureFinder::Evaluate_PeriodResidualAndDzdc_Direct     FeatureFinder.cpp:1661-1711
//   PTEvaluator::Eval                                        FeatureFinder.cpp:2313-2354
// written as the reference's straight loops (one candidate after another, or spread over `threads` std::threads).  The only
// arithmetic added to the oracle's is the HDRFloat<double> division (HDRFloat.h:624-636).  Records: include/fs_layout.h.
//
// Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC (tests/test_feature_finder_cpu.py).
#include "../../oracle/cpu_ref.cpp"

namespace {

enum { kRejected = 0, kOk = 1, kOkDirect = 2 }; // FS_FEATURE_* of include/fsmi355.h

template <class F> inline HT<F> HDivT(HT<F> a, HT<F> b) { return HT<F>{a.m / b.m, clampE(a.e - b.e)}; }

template <class F> struct FRec;
template <> struct FRec<float> {
    using In = fs_feature_in_hdr32;
    using Out = fs_feature_out_hdr32;
    using Real = fs_real_hdr32;
    static fs_cplx_hdr32 st(HCT<float> a) { return fs_cplx_hdr32{a.re, a.im, a.e}; }
    static fs_real_hdr32 st(HT<float> a) { return fs_real_hdr32{a.m, a.e}; }
};
template <> struct FRec<double> {
    using In = fs_feature_in_hdr64;
    using Out = fs_feature_out_hdr64;
    using Real = fs_real_hdr64;
    static fs_cplx_hdr64 st(HCT<double> a) { return fs_cplx_hdr64{a.re, a.im, a.e, 0}; }
    static fs_real_hdr64 st(HT<double> a) { return fs_real_hdr64{a.m, a.e, 0}; }
};

template <class F> struct Res {
    uint64_t period = 0;
    HCT<F> diff{}, dzdc{}, zcoeff{};
    HT<F> residual2{};
};

template <class F> inline HCT<F> CReduced(HCT<F> a)
{
    CReduce(a);
    return a;
}

// Evaluate_PT<FindPeriod>
template <class F, class IterT>
bool evaluate_pt(bool find, const typename Rec<F>::Orbit *orbit, uint64_t count, HCT<F> dc, HT<F> R, uint64_t maxIters,
                 uint64_t &ioPeriod, Res<F> &o)
{
    using H = HT<F>;
    using C = HCT<F>;
    const H zero = HZero<F>();
    const H one = Reduced(HFromNumber<F>(F(1.0)));
    const H two = Reduced(HFromNumber<F>(F(2.0)));
    const H escape2 = Reduced(HFromNumber<F>(F(4096.0)));
    CReduce(dc);
    if (count < 2)
        return false;
    const uint64_t cap = find ? maxIters : ioPeriod;
    if (cap < 1)
        return false;
    // scaleExp = 0: HdrLdexp(one, 0) = one
    const H ScalingFactor = one, InvScalingFactor = one;
    const C ScalingFactorC = CFromH(ScalingFactor, zero);
    const C InvScalingFactorC = CFromH(InvScalingFactor, zero);
    const H InvScale2 = Reduced(Mul(InvScalingFactor, InvScalingFactor));
    H SqrNearLinearRadius = zero, SqrNearLinearRadiusScale = zero;
    if (find) {
        R = Reduced(R);
        if (CmpPosReduced(R, zero) <= 0)
            return false;
        // PeriodicityPP::Init
        const H near1 = Reduced(HFromNumber<F>(F(0.25)));
        SqrNearLinearRadius = Reduced(Mul(R, R));
        SqrNearLinearRadiusScale = Reduced(Mul(near1, near1));
    }
    uint64_t refIteration = 0;
    C dz = CZero<F>(), z = CZero<F>();
    C dzdc = CZero<F>(), zcoeff = CZero<F>();
    for (uint64_t n = 0; n < cap; ++n) {
        zcoeff = n == 0 ? ScalingFactorC : CMul(zcoeff, CMulH(z, two));
        CReduce(zcoeff);
        dzdc = CAdd(CMul(dzdc, CMulH(z, two)), ScalingFactorC);
        CReduce(dzdc);
        const C zref = OrbitAt(orbit, refIteration);
        dz = CAdd(CMul(dz, CAdd(zref, z)), dc);
        CReduce(dz);
        refIteration++;
        z = CAdd(OrbitAt(orbit, refIteration), dz);
        CReduce(z);
        const H dzNorm = Reduced(CNormSq(dz));
        const H zNorm = Reduced(CNormSq(z));
        if (refIteration >= count - 1 || CmpPosReduced(zNorm, dzNorm) < 0) {
            dz = CReduced(z);
            refIteration = 0;
        }
        if (CmpPosReduced(zNorm, escape2) > 0)
            return false;
        if (find) {
            const H dzdcNormTrue = Reduced(Mul(Reduced(CNormSq(dzdc)), InvScale2));
            const IterT Iteration = (IterT)(n + 1);
            const H rhs = Reduced(Mul(SqrNearLinearRadius, dzdcNormTrue));
            if (CmpPosReduced(zNorm, rhs) < 0) {
                ioPeriod = Iteration;
                o.diff = CReduced(z);
                o.dzdc = CReduced(CMul(dzdc, InvScalingFactorC));
                o.zcoeff = CReduced(CMul(zcoeff, InvScalingFactorC));
                o.residual2 = zNorm;
                return true;
            }
            if (CmpPosReduced(dzdcNormTrue, zero) > 0) {
                const H lhsTight = Reduced(Mul(zNorm, SqrNearLinearRadiusScale));
                if (CmpPosReduced(lhsTight, rhs) < 0) {
                    const H newSqr = Reduced(HDivT(lhsTight, dzdcNormTrue));
                    if (CmpPosReduced(newSqr, zero) > 0)
                        SqrNearLinearRadius = newSqr;
                }
            }
        }
    }
    if (find)
        return false;
    o.diff = z;
    o.residual2 = Reduced(CNormSq(z));
    o.dzdc = CReduced(CMul(dzdc, InvScalingFactorC));
    o.zcoeff = CReduced(CMul(zcoeff, InvScalingFactorC));
    o.diff = CReduced(o.diff);
    return true;
}

// Evaluate_PeriodResidualAndDzdc_Direct
template <class F, class IterT> bool evaluate_direct(HCT<F> c, IterT period, Res<F> &o)
{
    using H = HT<F>;
    using C = HCT<F>;
    C z = CZero<F>(), dzdc = CZero<F>();
    const H one = Reduced(HFromNumber<F>(F(1.0)));
    const H two = Reduced(HFromNumber<F>(F(2.0)));
    const H escape2 = Reduced(HFromNumber<F>(F(4096.0)));
    C oneC = CFromH(one, HZero<F>());
    C zcoeff = CZero<F>();
    CReduce(oneC);
    for (IterT i = 0; i < period; ++i) {
        zcoeff = i == 0 ? CFromH(one, HZero<F>()) : CMul(zcoeff, CMulH(z, two));
        CReduce(zcoeff);
        dzdc = CAdd(CMul(dzdc, CMulH(z, two)), oneC);
        CReduce(dzdc);
        z = CAdd(CMul(z, z), c);
        CReduce(z);
        if (CmpPosReduced(Reduced(CNormSq(z)), escape2) > 0)
            return false;
    }
    o.diff = z;
    o.residual2 = Reduced(CNormSq(z));
    o.dzdc = dzdc;
    o.zcoeff = zcoeff;
    return true;
}

template <class F, class IterT>
void eval_one(bool find, const typename Rec<F>::Orbit *orbit, uint64_t count, HT<F> R, uint64_t maxIters,
              const typename FRec<F>::In &in, typename FRec<F>::Out &out)
{
    const HCT<F> dc{in.dc.re, in.dc.im, in.dc.e}, c{in.c.re, in.c.im, in.c.e};
    uint64_t period = find ? 0 : (uint64_t)(IterT)in.period;
    Res<F> r;
    uint32_t status = kRejected;
    if (evaluate_pt<F, IterT>(find, orbit, count, dc, R, maxIters, period, r))
        status = kOk;
    else if (!find && evaluate_direct<F, IterT>(c, (IterT)period, r))
        status = kOkDirect;
    typename FRec<F>::Out o{};
    if (status != kRejected) {
        o.status = status;
        o.period = period;
        o.diff = FRec<F>::st(r.diff);
        o.dzdc = FRec<F>::st(r.dzdc);
        o.zcoeff = FRec<F>::st(r.zcoeff);
        o.residual2 = FRec<F>::st(r.residual2);
    }
    out = o;
}

template <class F>
void eval_all(int iter_bytes, bool find, const void *orbit, uint64_t count, const void *radius, uint64_t maxIters,
              const void *in, void *out, uint64_t n, int threads)
{
    const auto *rad = (const typename FRec<F>::Real *)radius;
    const HT<F> R{rad->m, rad->e};
    const auto *orb = (const typename Rec<F>::Orbit *)orbit;
    const auto *ins = (const typename FRec<F>::In *)in;
    auto *outs = (typename FRec<F>::Out *)out;
    std::atomic<uint64_t> next{0};
    auto work = [&]() {
        for (uint64_t k; (k = next.fetch_add(1)) < n;) {
            if (iter_bytes == 8)
                eval_one<F, uint64_t>(find, orb, count, R, maxIters, ins[k], outs[k]);
            else
                eval_one<F, uint32_t>(find, orb, count, R, maxIters, ins[k], outs[k]);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; t++)
        pool.emplace_back(work);
    work();
    for (auto &t : pool)
        t.join();
}

} // namespace

// The checker of fs_feature_eval: same records, orbit = the fs_orbit_hdr32 / fs_orbit_hdr64 entries (count of them).
extern "C" void ffr_feature_eval(int is64, int iter_bytes, int mode, const void *radius, uint64_t max_iters, const void *orbit,
                                 uint64_t count, const void *in, void *out, uint64_t n, int threads)
{
    if (is64)
        eval_all<double>(iter_bytes, mode == 0, orbit, count, radius, max_iters, in, out, n, threads);
    else
        eval_all<float>(iter_bytes, mode == 0, orbit, count, radius, max_iters, in, out, n, threads);
}
