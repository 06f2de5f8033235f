// tests/feature/feature_direct_ref.cpp -- TEST INFRASTRUCTURE ONLY: CPU checker of the Feature Finder's Direct evaluator
// (fs_feature_eval_direct).
//
// An independent restatement, on the oracle's pinned HDRFloat arithmetic (through feature_ref.cpp, which includes
// oracle/cpu_ref.cpp as it is), of
//   FeatureFinder::Evaluate_FindPeriod_Direct               FeatureFinder.cpp:1576-1660
//   FeatureFinder::Evaluate_PeriodResidualAndDzdc_Direct    FeatureFinder.cpp:1661-1711   (evaluate_direct of feature_ref.cpp)
//   DirectEvaluator::Eval                                   FeatureFinder.cpp:2188-2211
// written as the reference's straight loops (one candidate after another, or spread over `threads` std::threads).
//
// Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC (tests/test_feature_direct_cpu.py).
#include "feature_ref.cpp"

#include <limits>

namespace {

// Evaluate_FindPeriod_Direct.  *steps (optional): loop trips taken, whatever the outcome.
template <class F, class IterT>
bool find_period_direct(HCT<F> c, uint64_t maxIters, HT<F> R, uint64_t &outPeriod, Res<F> &o, uint64_t *steps)
{
    using H = HT<F>;
    using C = HCT<F>;
    if (steps)
        *steps = 0;
    R = Reduced(R);
    const H zero = HZero<F>();
    if (CmpPosReduced(R, zero) <= 0)
        return false;
    const H two = Reduced(HFromNumber<F>(F(2.0)));
    const H one = Reduced(HFromNumber<F>(F(1.0)));
    const H escape2 = Reduced(HFromNumber<F>(F(4096.0)));
    const H R2 = Reduced(Mul(R, R));
    C z = CZero<F>(), dzdc = CZero<F>(), zcoeff = CZero<F>();
    for (uint64_t n = 0; n < maxIters; ++n) {
        if (steps)
            *steps = n + 1;
        zcoeff = n == 0 ? CFromH(one, HZero<F>()) : CMul(zcoeff, CMulH(z, two));
        CReduce(zcoeff);
        dzdc = CAdd(CMul(dzdc, CMulH(z, two)), CFromH(one, HZero<F>()));
        CReduce(dzdc);
        z = CAdd(CMul(z, z), c);
        CReduce(z);
        const H z2 = Reduced(CNormSq(z));
        if (CmpPosReduced(z2, escape2) > 0)
            break;
        const H d2 = Reduced(CNormSq(dzdc));
        const H rhs = Reduced(Mul(R2, d2));
        if (CmpPosReduced(z2, rhs) < 0) {
            const uint64_t cand = n + 1;
            if (cand <= (uint64_t)std::numeric_limits<IterT>::max()) {
                outPeriod = (uint64_t)(IterT)cand;
                o.diff = z;
                o.dzdc = dzdc;
                o.zcoeff = zcoeff;
                o.residual2 = z2;
                return true;
            }
            return false;
        }
    }
    return false;
}

template <class F, class IterT>
void eval_one_direct(bool find, HT<F> R, uint64_t maxIters, const typename FRec<F>::In &in, typename FRec<F>::Out &out,
                     uint64_t *steps)
{
    const HCT<F> c{in.c.re, in.c.im, in.c.e};
    uint64_t period = find ? 0 : (uint64_t)(IterT)in.period;
    Res<F> r;
    bool ok;
    if (find) {
        ok = find_period_direct<F, IterT>(c, maxIters, R, period, r, steps);
    } else {
        ok = evaluate_direct<F, IterT>(c, (IterT)period, r);
        if (steps)
            *steps = period;
    }
    typename FRec<F>::Out o{};
    if (ok) {
        o.status = kOkDirect;
        o.period = period;
        o.diff = FRec<F>::st(r.diff);
        o.dzdc = FRec<F>::st(r.dzdc);
        o.zcoeff = FRec<F>::st(r.zcoeff);
        o.residual2 = FRec<F>::st(r.residual2);
    }
    out = o;
}

template <class F>
void eval_all_direct(int iter_bytes, bool find, const void *radius, uint64_t maxIters, const void *in, void *out, uint64_t n,
                     int threads, uint64_t *steps)
{
    const auto *rad = (const typename FRec<F>::Real *)radius;
    const HT<F> R{rad->m, rad->e};
    const auto *ins = (const typename FRec<F>::In *)in;
    auto *outs = (typename FRec<F>::Out *)out;
    std::atomic<uint64_t> next{0};
    auto work = [&]() {
        // (in runs of 64: a candidate of a period search is short)
        for (uint64_t b; (b = next.fetch_add(64)) < n;)
            for (uint64_t k = b; k < n && k < b + 64; ++k) {
                uint64_t *st = steps ? steps + k : nullptr;
                if (iter_bytes == 8)
                    eval_one_direct<F, uint64_t>(find, R, maxIters, ins[k], outs[k], st);
                else
                    eval_one_direct<F, uint32_t>(find, R, maxIters, ins[k], outs[k], st);
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

// The checker of fs_feature_eval_direct: same records.
extern "C" void ffr_feature_eval_direct(int is64, int iter_bytes, int mode, const void *radius, uint64_t max_iters, const void *in,
                                        void *out, uint64_t n, int threads)
{
    if (is64)
        eval_all_direct<double>(iter_bytes, mode == 0, radius, max_iters, in, out, n, threads, nullptr);
    else
        eval_all_direct<float>(iter_bytes, mode == 0, radius, max_iters, in, out, n, threads, nullptr);
}

// The same, and steps[k] = the loop trips candidate k took (measurements: how unevenly the lanes of a wave finish).
extern "C" void ffr_feature_eval_direct_steps(int is64, int iter_bytes, int mode, const void *radius, uint64_t max_iters,
                                              const void *in, void *out, uint64_t n, int threads, uint64_t *steps)
{
    if (is64)
        eval_all_direct<double>(iter_bytes, mode == 0, radius, max_iters, in, out, n, threads, steps);
    else
        eval_all_direct<float>(iter_bytes, mode == 0, radius, max_iters, in, out, n, threads, steps);
}
