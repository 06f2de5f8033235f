// tests/feature/feature_plain_ref.cpp -- TEST INFRASTRUCTURE ONLY: CPU checker of the plain-type Feature Finder evaluators
// (fs_feature_eval_plain, fs_feature_eval_plain_direct), T = float / double.
//
// Written from the reference as its straight loops over one candidate at a time, in plain C++ arithmetic; it includes nothing of
// the product or of oracle/ (the records are declared again below, sizes asserted):
//   FeatureFinder::Evaluate_PT<true | false>                 FeatureFinder.cpp:1757-1921
//   PeriodicityPP::Init / CheckPeriodicity                   FeatureFinder.cpp:1471-1534
//   FeatureFinder::Evaluate_FindPeriod_Direct                FeatureFinder.cpp:1576-1660
//   FeatureFinder::Evaluate_PeriodResidualAndDzdc_Direct     FeatureFinder.cpp:1661-1711
//   PTEvaluator::Eval / DirectEvaluator::Eval                FeatureFinder.cpp:2313-2354, 2188-2211
//   FloatComplex<T>                                          FloatComplex.h:174-229, 302-305
//   RuntimeDecompressor::GetCompressedComplex                PerturbationResultsHelpers.h:35-199 (the waypoint path)
// The orbit is either the expanded array of {x, y} entries or the waypoints {index, x, y} with the decompressor's constant,
// which a per-candidate decompressor object then serves by index, as results.GetComplex(dec, refIteration) does.
//
// Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC (tests/test_feature_plain_cpu.py).  x86-64 SSE2 arithmetic: every
// operator is one IEEE operation in T, subnormals kept.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

enum { STATUS_REJECTED = 0, STATUS_PT = 1, STATUS_DIRECT = 2 };

template <class T> struct RecIn {
    T dc[2];
    T c[2];
    uint64_t period;
};
template <class T> struct RecOut {
    uint32_t status;
    uint32_t pad0;
    uint64_t period;
    T diff[2];
    T dzdc[2];
    T zcoeff[2];
    T residual2;
    // (the compiler pads the float record to 48 bytes; the record is zero-filled before it is written)
};
static_assert(sizeof(RecIn<float>) == 24 && sizeof(RecIn<double>) == 40, "input records");
static_assert(sizeof(RecOut<float>) == 48 && sizeof(RecOut<double>) == 72, "output records");

template <class T> struct Entry {
    T x, y;
};
template <class T> struct Waypoint {
    uint64_t index_and_rebase;
    T x, y;
};
static_assert(sizeof(Waypoint<float>) == 16 && sizeof(Waypoint<double>) == 24, "waypoints");

// FloatComplex<T>
template <class T> struct Cx {
    T re{}, im{};
    Cx() = default;
    Cx(T r, T i) : re(r), im(i) {}
    Cx &operator+=(const Cx &o)
    {
        re = re + o.re;
        im = im + o.im;
        return *this;
    }
    Cx &operator*=(const Cx &f)
    {
        const T r = (re * f.re) - (im * f.im);
        const T i = (re * f.im) + (im * f.re);
        re = r;
        im = i;
        return *this;
    }
    Cx &operator*=(T f)
    {
        re *= f;
        im *= f;
        return *this;
    }
    T norm_squared() const { return T(re * re + im * im); }
};
template <class T> Cx<T> operator+(Cx<T> a, const Cx<T> &b) { return a += b; }
template <class T> Cx<T> operator*(Cx<T> a, const Cx<T> &b) { return a *= b; }
template <class T> Cx<T> operator*(Cx<T> a, T b) { return a *= b; }

// What Evaluate_PT reads the orbit through: GetComplex(index).
template <class T> struct ExpandedSource {
    const Entry<T> *z;
    Cx<T> get(uint64_t i) { return Cx<T>(z[i].x, z[i].y); }
};

// The decompressor: keeps the last value it produced; the next index costs one iteration (or one waypoint), any other index a
// search for the last waypoint at or before it and the iterations from there.  IterT-wide positions.
template <class T, class IterT> struct WaypointSource {
    const Waypoint<T> *wp;
    uint64_t n_wp;
    T cx, cy;
    bool have = false;
    IterT at = 0;      // index of (zx, zy)
    uint64_t next = 0; // first waypoint behind `at`
    T zx{}, zy{};

    IterT index(uint64_t k) const { return (IterT)(wp[k].index_and_rebase & 0x7FFFFFFFFFFFFFFFull); }
    void advance()
    {
        at++;
        if (next < n_wp && index(next) == at) {
            zx = wp[next].x;
            zy = wp[next].y;
            next++;
            return;
        }
        const T old = zx;
        zx = zx * zx - zy * zy + cx;
        zy = T(2.0f) * old * zy + cy;
    }
    Cx<T> get(uint64_t i64)
    {
        const IterT i = (IterT)i64;
        if (!have || i < at) {
            uint64_t lo = 0, hi = n_wp; // last waypoint with index <= i
            while (hi - lo > 1) {
                const uint64_t mid = lo + (hi - lo) / 2;
                (index(mid) <= i ? lo : hi) = mid;
            }
            zx = wp[lo].x;
            zy = wp[lo].y;
            at = index(lo);
            next = lo + 1;
            have = true;
        }
        while (at < i)
            advance();
        return Cx<T>(zx, zy);
    }
};

template <class T> struct Result {
    uint64_t period = 0;
    Cx<T> diff, dzdc, zcoeff;
    T residual2{};
};

template <class T, class IterT, class Source>
bool evaluate_pt(bool findPeriod, Source &orbit, uint64_t refOrbitLength, const Cx<T> dc, T R, uint64_t maxIters,
                 uint64_t &ioPeriod, Result<T> &out)
{
    using C = Cx<T>;
    const T zero = T{}, one = T{1.0}, two = T{2.0}, escape2 = T{4096.0};
    if (refOrbitLength < 2)
        return false;
    const uint64_t cap = findPeriod ? maxIters : ioPeriod;
    if (cap < 1)
        return false;
    const T ScalingFactor = one, InvScalingFactor = one; // HdrLdexp(one, -0), HdrLdexp(one, 0)
    const C ScalingFactorC(ScalingFactor, T{}), InvScalingFactorC(InvScalingFactor, T{});
    const T InvScale2 = InvScalingFactor * InvScalingFactor;
    T SqrNearLinearRadius{}, SqrNearLinearRadiusScale{};
    if (findPeriod) {
        if (R <= zero)
            return false;
        const T near1 = T{0.25};
        SqrNearLinearRadius = R * R;
        SqrNearLinearRadiusScale = near1 * near1;
    }
    uint64_t refIteration = 0;
    C dz, z, dzdc, zcoeff;
    for (uint64_t n = 0; n < cap; ++n) {
        if (n == 0)
            zcoeff = ScalingFactorC;
        else
            zcoeff = zcoeff * (z * two);
        dzdc = dzdc * (z * two) + ScalingFactorC;
        const C zref = orbit.get(refIteration);
        dz = dz * (zref + z) + dc;
        refIteration++;
        const C zrefNext = orbit.get(refIteration);
        z = zrefNext + dz;
        const T dzNorm = dz.norm_squared();
        const T zNorm = z.norm_squared();
        if (refIteration >= refOrbitLength - 1 || zNorm < dzNorm) {
            dz = z;
            refIteration = 0;
        }
        if (zNorm > escape2)
            return false;
        if (findPeriod) {
            const T dzdcNormStored = dzdc.norm_squared();
            const T dzdcNormTrue = dzdcNormStored * InvScale2;
            const IterT Iteration = (IterT)(n + 1);
            // CheckPeriodicity
            const T rhs = SqrNearLinearRadius * dzdcNormTrue;
            if (zNorm < rhs) {
                ioPeriod = Iteration;
                out.diff = z;
                out.dzdc = dzdc * InvScalingFactorC;
                out.zcoeff = zcoeff * InvScalingFactorC;
                out.residual2 = zNorm;
                return true;
            }
            if (dzdcNormTrue > zero) {
                const T lhsTight = zNorm * SqrNearLinearRadiusScale;
                if (lhsTight < rhs) {
                    const T newSqr = lhsTight / dzdcNormTrue;
                    if (newSqr > zero)
                        SqrNearLinearRadius = newSqr;
                }
            }
        }
    }
    if (findPeriod)
        return false;
    out.diff = z;
    out.residual2 = z.norm_squared();
    out.dzdc = dzdc * InvScalingFactorC;
    out.zcoeff = zcoeff * InvScalingFactorC;
    return true;
}

template <class T, class IterT> bool find_period_direct(const Cx<T> c, uint64_t maxIters, T R, uint64_t &outPeriod, Result<T> &out)
{
    using C = Cx<T>;
    if (R <= T{})
        return false;
    const T two = T{2.0}, one = T{1.0}, escape2 = T{4096.0};
    const T R2 = R * R;
    C z, dzdc, zcoeff;
    for (uint64_t n = 0; n < maxIters; ++n) {
        if (n == 0)
            zcoeff = C(one, T{});
        else
            zcoeff = zcoeff * (z * two);
        dzdc = dzdc * (z * two) + C(one, T{});
        z = (z * z) + c;
        const T z2 = z.norm_squared();
        if (z2 > escape2)
            break;
        const T d2 = dzdc.norm_squared();
        const T rhs = R2 * d2;
        if (z2 < rhs) {
            const uint64_t cand = n + 1;
            if (cand <= (uint64_t)(IterT)~(IterT)0) {
                outPeriod = (uint64_t)(IterT)cand;
                out.diff = z;
                out.dzdc = dzdc;
                out.zcoeff = zcoeff;
                out.residual2 = z2;
                return true;
            }
            return false;
        }
    }
    return false;
}

template <class T, class IterT> bool residual_direct(const Cx<T> c, IterT period, Result<T> &out)
{
    using C = Cx<T>;
    C z, dzdc, zcoeff;
    const T one = T{1.0}, two = T{2.0}, escape2 = T{4096.0};
    const C oneC(one, T{});
    for (IterT i = 0; i < period; ++i) {
        if (i == 0)
            zcoeff = C(one, T{});
        else
            zcoeff = zcoeff * (z * two);
        dzdc = dzdc * (z * two) + oneC;
        z = (z * z) + c;
        if (z.norm_squared() > escape2)
            return false;
    }
    out.diff = z;
    out.residual2 = z.norm_squared();
    out.dzdc = dzdc;
    out.zcoeff = zcoeff;
    return true;
}

template <class T> void write_out(void *dst, uint32_t status, uint64_t period, const Result<T> &r)
{
    unsigned char raw[sizeof(RecOut<T>)];
    memset(raw, 0, sizeof(raw));
    if (status != STATUS_REJECTED) {
        RecOut<T> o;
        memset(&o, 0, sizeof(o));
        o.status = status;
        o.period = period;
        o.diff[0] = r.diff.re, o.diff[1] = r.diff.im;
        o.dzdc[0] = r.dzdc.re, o.dzdc[1] = r.dzdc.im;
        o.zcoeff[0] = r.zcoeff.re, o.zcoeff[1] = r.zcoeff.im;
        o.residual2 = r.residual2;
        memcpy(raw, &o, sizeof(o));
    }
    memcpy(dst, raw, sizeof(raw));
}

struct Job {
    int iter_bytes, mode;
    const void *radius;
    uint64_t max_iters;
    const void *orbit; // Entry<T>[count], or NULL: the waypoints
    uint64_t count;
    const void *wp;
    uint64_t n_wp;
    const void *c_low; // T[2]
    bool direct;
    const void *in;
    void *out;
    uint64_t n;
};

template <class T, class IterT> void one_candidate(const Job &j, uint64_t k)
{
    const RecIn<T> &in = ((const RecIn<T> *)j.in)[k];
    const bool find = j.mode == 0;
    const T R = *(const T *)j.radius;
    const Cx<T> dc(in.dc[0], in.dc[1]), c(in.c[0], in.c[1]);
    uint64_t period = find ? 0 : (uint64_t)(IterT)in.period;
    Result<T> r;
    uint32_t status = STATUS_REJECTED;
    if (j.direct) {
        if (find ? find_period_direct<T, IterT>(c, j.max_iters, R, period, r) : residual_direct<T, IterT>(c, (IterT)period, r))
            status = STATUS_DIRECT;
    } else {
        bool ok;
        if (j.orbit) {
            ExpandedSource<T> src{(const Entry<T> *)j.orbit};
            ok = evaluate_pt<T, IterT>(find, src, j.count, dc, R, j.max_iters, period, r);
        } else {
            WaypointSource<T, IterT> src{(const Waypoint<T> *)j.wp, j.n_wp, ((const T *)j.c_low)[0], ((const T *)j.c_low)[1]};
            ok = evaluate_pt<T, IterT>(find, src, j.count, dc, R, j.max_iters, period, r);
        }
        if (ok)
            status = STATUS_PT;
        else if (!find && residual_direct<T, IterT>(c, (IterT)period, r))
            status = STATUS_DIRECT;
    }
    write_out<T>((char *)j.out + k * sizeof(RecOut<T>), status, period, r);
}

void run(int is64, const Job &j, int threads)
{
    std::atomic<uint64_t> next{0};
    auto work = [&]() {
        for (uint64_t k; (k = next.fetch_add(1)) < j.n;) {
            if (is64)
                j.iter_bytes == 8 ? one_candidate<double, uint64_t>(j, k) : one_candidate<double, uint32_t>(j, k);
            else
                j.iter_bytes == 8 ? one_candidate<float, uint64_t>(j, k) : one_candidate<float, uint32_t>(j, k);
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

// The checker of fs_feature_eval_plain.  orbit = count fs_orbit_f32 / fs_orbit_f64 entries; or NULL, and then wp = n_wp
// fs_orbit_f32_rc / fs_orbit_f64_rc waypoints with c_low = {OrbitXLow, OrbitYLow} in T, count = the uncompressed length.
extern "C" void fpr_feature_eval(int is64, int iter_bytes, int mode, const void *radius, uint64_t max_iters, const void *orbit,
                                 uint64_t count, const void *wp, uint64_t n_wp, const void *c_low, const void *in, void *out,
                                 uint64_t n, int threads)
{
    run(is64, Job{iter_bytes, mode, radius, max_iters, orbit, count, wp, n_wp, c_low, false, in, out, n}, threads);
}

// The checker of fs_feature_eval_plain_direct.
extern "C" void fpr_feature_eval_direct(int is64, int iter_bytes, int mode, const void *radius, uint64_t max_iters, const void *in,
                                        void *out, uint64_t n, int threads)
{
    run(is64, Job{iter_bytes, mode, radius, max_iters, nullptr, 0, nullptr, 0, nullptr, true, in, out, n}, threads);
}
