// inputs_state.hpp -- what the units of libfsinputs.so share: host-side builders for the *inputs* of the per-pixel pass
// (C ABI: include/fs_inputs.h).  Internal to fractalshark_amd/host/.
//
// The MI355X renderer consumes what FractalShark's host code already produces: a view (bounding box ->
// dx/dy/centre), a reference orbit (PerturbationResults layout) and an LAv2 table (LAReference layout).
// On a FractalShark host these come from Fractal.cpp / RefOrbitCalc.cpp / LAReference.cpp; this file is
// the stand-alone equivalent used by bench.py, the tests and the oracle harness, so that the whole
// pipeline can run where FractalShark itself is not built.  It is upstream of the hot path (SURVEY.md
// section 8(f) rows 1-3), host-only, single-threaded, and follows the reference call-for-call on GMP's
// mpf_t so the extracted float/double values are the reference's:
//
//   view.cpp          FractalViewPresets.cpp GetViewPreset, PointZoomBBConverter.cpp:26-53,100-117,271-330,
//                     PrecisionCalculator.cpp:58-108, Fractal.cpp:264-307,591-629;
//                     coords: Fractal.cpp:2118-2119 (direct), :2230-2238 / :2513-2521 (perturbation)
//   im_files.cpp      RefOrbitCalc.cpp:3039-3166,3425-3520, PerturbationResults.cpp:1347-1850,2013-2211
//   orbit_hdr.cpp     RefOrbitCalc.cpp:244-249,423-647 (ST / STPeriodicity), PerturbationResults.cpp:812-884
//   convert_2x32.cpp  PerturbationResults.cpp:239-347, LAReference.h:163-213, dblflt.h:37-52
//   la_table.cpp      LAReference.cpp:28-210 (stage 0, single-threaded), :215-770 (stage 0, multi-threaded
//                     hand-off, replayed sequentially), :774-966 (higher stages), :971-1013, :1050-1074 (AT);
//                     LAInfoDeep.h:108-391,456-506; LAParameters.h:66-75
//   bla_table.cpp     BLAS.cpp:25-255, BLA.cuh:7-110
//   plain_inputs.cpp  the floatOrDouble arms of RefOrbitCalc.cpp:423-647; BLAS.cpp with T = double
//   feature_scan.cpp  FeatureFinderOrchestrator.cpp:485-559, FeatureFinder.cpp:2443-2697
#pragma once
#include <gmp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../csrc/hdr_math.hpp"
#include "../csrc/df32_math.hpp"
#include "../csrc/la_math.hpp"
#include "../csrc/bla_math.hpp"
#include "../../include/fs_inputs.h"

using namespace fs;
using namespace fs::la;

// ------------------------------------------------------------------ mpf wrapper (HighPrecision.h)
// Mirrors HighPrecisionT: values carry their own precision; binary operators produce a result with the
// precision of the left operand (HighPrecision.h:262-300); default-constructed values use
// mpf_get_default_prec().
struct Mp {
    mpf_t v;
    Mp() { mpf_init(v); }
    explicit Mp(uint64_t prec_bits, int) { mpf_init2(v, prec_bits); }
    Mp(const Mp &o)
    {
        mpf_init2(v, mpf_get_prec(o.v));
        mpf_set(v, o.v);
    }
    Mp &operator=(const Mp &o)
    {
        if (this != &o) {
            mpf_set_prec(v, mpf_get_prec(o.v));
            mpf_set(v, o.v);
        }
        return *this;
    }
    ~Mp() { mpf_clear(v); }
    static Mp from_str(const char *s)
    {
        Mp r;
        mpf_set_str(r.v, s, 10);
        return r;
    }
    static Mp from_ui(uint64_t x)
    {
        Mp r;
        mpf_set_ui(r.v, x);
        return r;
    }
    uint64_t prec() const { return (uint32_t)mpf_get_prec(v); }
    void set_prec(uint64_t p) { mpf_set_prec(v, p); }
};

inline Mp operator+(const Mp &a, const Mp &b)
{
    Mp r(a.prec(), 0);
    mpf_add(r.v, a.v, b.v);
    return r;
}
inline Mp operator-(const Mp &a, const Mp &b)
{
    Mp r(a.prec(), 0);
    mpf_sub(r.v, a.v, b.v);
    return r;
}
inline Mp operator/(const Mp &a, const Mp &b)
{
    Mp r(a.prec(), 0);
    mpf_div(r.v, a.v, b.v);
    return r;
}
inline Mp mp_abs(const Mp &a)
{
    Mp r(a.prec(), 0);
    mpf_abs(r.v, a.v);
    return r;
}

// HDRFloat(const mpf_t) -- HDRFloat.h:366-389: mantissa in [0.5,1) as returned by mpf_get_d_2exp, cast
// to F; NOT reduced.  Zero -> default.
template <class F> hreal<F> hr_from_mpf(const mpf_t x)
{
    if (mpf_cmp_ui(x, 0) == 0)
        return hr_zero<F>();
    long e;
    const double d = mpf_get_d_2exp(&e, x);
    return hreal<F>{(F)d, (int32_t)e};
}

// The reference orbit's high-precision iteration z <- z^2 + c from z = c (RefOrbitCalc.cpp:423-647).  Every value is
// mpf_init'ed, so it has the DEFAULT precision: construct after mpf_set_default_prec(the view's precision bits).
struct MpStepper {
    mpf_t cx, cy, zx, zy, zx2, t1, t2;
    MpStepper(const Mp &cx0, const Mp &cy0)
    {
        for (mpf_ptr p : {cx, cy, zx, zy, zx2, t1, t2})
            mpf_init(p);
        mpf_set(cx, cx0.v);
        mpf_set(cy, cy0.v);
        mpf_set(zx, cx);
        mpf_set(zy, cy);
    }
    MpStepper(const MpStepper &) = delete;
    ~MpStepper()
    {
        for (mpf_ptr p : {cx, cy, zx, zy, zx2, t1, t2})
            mpf_clear(p);
    }
    void step()
    {
        mpf_mul_2exp(zx2, zx, 1);
        mpf_mul(t1, zx, zx);
        mpf_mul(t2, zy, zy);
        mpf_sub(zx, t1, t2);
        mpf_add(zx, zx, cx);
        mpf_mul(zy, zx2, zy);
        mpf_add(zy, zy, cy);
    }
};

// ------------------------------------------------------------------ view (view.cpp)
struct fsh_view {
    Mp minX, minY, maxX, maxY, ptX, ptY, zoom;
    uint64_t prec_bits = 0;
    uint32_t width = 0, height = 0;
};
// The rest of what the reference does to a new view: the box form of PointZoomBBConverter (from_box; the point + zoom form
// has set ptX / ptY / zoom already), Fractal::SetPrecision, SquareAspectRatio.
fsh_view *finish_view(std::unique_ptr<fsh_view> vw, bool from_box);

// ------------------------------------------------------------------ reference orbit (orbit_hdr.cpp)
template <class F> struct OrbitT {
    std::vector<hreal<F>> x, y; // entry 0 is the explicit zero entry
    uint64_t period = 0;
    hreal<F> maxRadius{};
    hreal<F> orbitXLow{}, orbitYLow{};
    Mp cx, cy; // reference point (m_OrbitX / m_OrbitY)
    uint64_t prec_bits = 0;
    // PerturbExtras::Bad flag per entry (RefOrbitCalc.cpp:550-562,625-627); computed for every orbit, only the scaled
    // kernels read it
    std::vector<uint8_t> bad;
    // packed copies in the ABI layout, built lazily
    std::vector<fs_orbit_hdr32> packed32;
    std::vector<fs_orbit_hdr64> packed64;
    std::vector<fs_orbit_hdr32_bad> packed32_bad;
    std::vector<fs_orbit_f32_bad> packed_f32_bad;
    // PerturbExtras::SimpleCompression: waypoints (m_FullOrbit of the compressed PerturbationResults); x / y above
    // then hold the orbit as RuntimeDecompressor reproduces it.
    bool compressed = false;
    std::vector<uint64_t> wp_index;
    std::vector<hreal<F>> wp_x, wp_y;
    std::vector<fs_orbit_hdr32_rc> packed_rc32;
    std::vector<fs_orbit_hdr64_rc> packed_rc64;
};

struct fsh_orbit {
    int is64 = 0;
    OrbitT<float> f;
    OrbitT<double> d;
};

// RuntimeDecompressor::GetCompressedComplex's runOneIter, PerturbationResultsHelpers.h:51-58 (== the compressor's own
// advance, PerturbationResults.cpp:2374-2378).
template <class F> void rc_one_iter(hreal<F> &zx, hreal<F> &zy, hreal<F> cxLow, hreal<F> cyLow)
{
    const hreal<F> zx_old = zx;
    zx = hr_add(hr_sub(hr_mul(zx, zx), hr_mul(zy, zy)), cxLow);
    hr_reduce(zx);
    zy = hr_add(hr_mul(hr_mul(hr_from_number<F>(F(2)), zx_old), zy), cyLow);
    hr_reduce(zy);
}

// ------------------------------------------------------------------ plain float / double orbit (plain_inputs.cpp)
// PerturbationResults<uint32_t, T, Disable> for a plain T (only what the LA builder reads)
template <class T> struct PlainOrbit {
    std::vector<preal<T>> x, y; // entry 0 = {0, 0}
    uint64_t period = 0;
    preal<T> maxRadius{};
    Mp cx, cy;
    // PerturbExtras::SimpleCompression: waypoints; x / y then hold the orbit as RuntimeDecompressor reproduces it
    bool compressed = false;
    std::vector<uint64_t> wp_index;
    std::vector<T> wp_x, wp_y;
    // PerturbExtras::Bad flag per entry (RefOrbitCalc.cpp:550-562,625-627), in double arithmetic; only fsh_orbit_f64 reads it
    std::vector<uint8_t> bad;
    T orbitXLow{}, orbitYLow{};
};
// runOneIter for a plain T (PerturbationResultsHelpers.h:51-58; HdrReduce is the identity)
template <class T> void rc_one_iter_plain(T &zx, T &zy, T cxLow, T cyLow)
{
    const T zx_old = zx;
    zx = zx * zx - zy * zy + cxLow;
    zy = T(2.0f) * zx_old * zy + cyLow;
}
// (F is a number family of la_math.hpp: float / double = HDRFloat<F>, plain<float> / plain<double> = the type itself --
// the reference's CompressMax / DecompressMax are one template over T, with HdrReduce a no-op, HdrAbs = fabs and
// HdrMaxReduced = `(one > two) ? one : two` for a plain T, HDRFloat.h:1385-1500)
template <class T> preal<T> hr_add(preal<T> a, preal<T> b) { return preal<T>{a.m + b.m}; }
template <class T> preal<T> hr_sub(preal<T> a, preal<T> b) { return preal<T>{a.m - b.m}; }
template <class T> preal<T> hr_abs(preal<T> a) { return preal<T>{std::fabs(a.m)}; }
template <class T> int hr_cmp(preal<T> a, preal<T> b) { return a.m > b.m ? 1 : (a.m < b.m ? -1 : 0); }
template <class T> void rc_one_iter(preal<T> &zx, preal<T> &zy, preal<T> cxLow, preal<T> cyLow)
{
    rc_one_iter_plain(zx.m, zy.m, cxLow.m, cyLow.m);
}

// ------------------------------------------------------------------ LAv2 table (la_table.cpp)
// (the record arithmetic -- LAParams, the number families, LAInfo, la_init / la_step / la_composite / la_detect_period,
// ATInfoT, la_create_at, at_usable -- lives in csrc/la_math.hpp, shared with the device builder)
template <class F> struct LATable {
    std::vector<LAInfo<F>> las;
    std::vector<fs_la_stage_u32> stages; // only [0, stageCount) meaningful
    uint32_t stageCount = 0;
    bool useAT = false;
    bool isValid = false;
    ATInfoT<F> at;
    std::vector<fs_la_hdr32_u32> packed32;
    std::vector<fs_la_stage_u32> packedStages;
};
template <class F> struct orbit_of {
    using type = OrbitT<F>;
};
template <class T> struct orbit_of<plain<T>> {
    using type = PlainOrbit<T>;
};
// LAReference::GenerateApproximationData into t, packedStages included.  LABuilder<F> is compiled in la_table.cpp alone:
// F = float, double, plain<float>, plain<double> are instantiated there.
template <class F>
void la_generate(const typename orbit_of<F>::type &ob, LATable<F> &t, int host_threads, bool use_small_exponents = false);

struct fsh_la {
    int is64 = 0;
    LATable<float> t32;
    LATable<double> t64;
    std::vector<fs_la_hdr64_u32> packed64;
};

// ------------------------------------------------------------------ BLA table (bla_table.cpp, plain_inputs.cpp)
// BLAS::Init, BLAS.cpp:212-255, over any record type: one_step(m) = BLAS::CreateOneStep (:74-93) and merge(x, y) =
// BLAS::MergeTwoBlas (:25-47) supply the arithmetic.  The reference fills level 2 and merges upwards on several threads; every
// element is a pure function of the orbit, so a sequential fill gives the same table.  Returns m_LM2.
template <class Rec, class OneStep, class Merge>
int32_t bla_pyramid(size_t InM, std::vector<std::vector<Rec>> &B, OneStep one_step, Merge merge)
{
    constexpr size_t kFirstLevel = 2; // BLAS.h:22
    size_t m = InM - 1;
    if (InM == 0 || m == 0)
        return 0;
    std::vector<size_t> elementsPerLevel;
    for (; m > 1; m = (m + 1) >> 1)
        elementsPerLevel.push_back(m);
    elementsPerLevel.push_back(m);
    const size_t L = elementsPerLevel.size();
    B.clear();
    B.resize(L);
    const int32_t LM2 = (int32_t)L - 2 < 0 ? 0 : (int32_t)L - 2;
    if (kFirstLevel >= L)
        return LM2;
    for (size_t l = kFirstLevel; l < L; l++)
        B[l].resize(elementsPerLevel[l]);
    // BLAS::CreateLStep, BLAS.cpp:49-72
    auto l_step = [&](auto &self, size_t level, size_t mm) -> Rec {
        if (level == 0)
            return one_step(mm);
        const size_t m2 = mm << 1, mx = m2 - 1, my = m2, levelm1 = level - 1;
        if (my <= elementsPerLevel[levelm1]) {
            const Rec x = self(self, levelm1, mx);
            const Rec y = self(self, levelm1, my);
            return merge(x, y);
        }
        return self(self, levelm1, mx);
    };
    // InitInternal, BLAS.cpp:97-139
    const size_t elements = elementsPerLevel[kFirstLevel] + 1;
    for (size_t mm = 1; mm < elements; mm++)
        B[kFirstLevel][mm - 1] = l_step(l_step, kFirstLevel, mm);
    // Merge, BLAS.cpp:141-210
    size_t src = kFirstLevel;
    const size_t maxLevel = elementsPerLevel.size() - 1;
    for (size_t elementsSrc = elementsPerLevel[src]; src < maxLevel && elementsSrc > 1; src++) {
        const size_t dst = src + 1;
        const size_t elementsDst = elementsPerLevel[dst];
        for (size_t k = 0; k < elementsDst; k++) {
            const size_t mx = k << 1, my = mx + 1;
            if (my < elementsSrc)
                B[dst][k] = merge(B[src][mx], B[src][my]);
            else
                B[dst][k] = B[src][mx];
        }
        elementsSrc = elementsDst;
    }
    return LM2;
}
// the per-level pointers and sizes the C ABI hands out (levels below m_FirstLevel: NULL, 0)
template <class Rec>
void bla_export(const std::vector<std::vector<Rec>> &levels, std::vector<const void *> &ptrs, std::vector<uint64_t> &sizes)
{
    for (const auto &lv : levels) {
        ptrs.push_back(lv.empty() ? nullptr : (const void *)lv.data());
        sizes.push_back(lv.size());
    }
}

struct fsh_bla {
    int is64 = 0;
    std::vector<std::vector<fs_bla_hdr32>> levels32;
    std::vector<std::vector<fs_bla_hdr64>> levels64;
    std::vector<const void *> ptrs;
    std::vector<uint64_t> sizes;
    int32_t lm2 = 0;
};

// ------------------------------------------------------------------ plain inputs (plain_inputs.cpp)
template <class T> struct plain_recs;
template <> struct plain_recs<float> {
    using orbit_rc = fs_orbit_f32_rc;
    using orbit = fs_orbit_f32;
    using la = fs_la_f32_u32;
    using at = fs_at_f32_u32;
    using cplx = fs_cplx_f32;
};
template <> struct plain_recs<double> {
    using orbit_rc = fs_orbit_f64_rc;
    using orbit = fs_orbit_f64;
    using la = fs_la_f64_u32;
    using at = fs_at_f64_u32;
    using cplx = fs_cplx_f64;
};

template <class T> struct PlainInputs {
    PlainOrbit<T> ob;
    LATable<plain<T>> t;
    std::vector<typename plain_recs<T>::orbit> orbit_packed;
    std::vector<typename plain_recs<T>::orbit_rc> rc_packed; // GPUReferenceIter<T, SimpleCompression>[]
    std::vector<typename plain_recs<T>::la> la_packed;
    typename plain_recs<T>::at at_packed;

    void build(const fsh_view &vw, uint64_t max_iter, int periodicity, int host_threads, int compression_exp);
    // everything derived from the orbit (packed records, LA table, ATInfo): also what a loaded ".im" orbit goes through
    void finish(int host_threads);
};

struct fsh_plain {
    int kind = 0; // 0 float, 1 double
    PlainInputs<float> f;
    PlainInputs<double> d;
};

// PerturbationResults<uint32_t,double,Disable> + BLAS<uint32_t,double>
struct fsh_orbit_f64 {
    PlainOrbit<double> ob;
    std::vector<fs_orbit_f64> z; // the orbit in the ABI layout, entry 0 = {0,0}
    std::vector<fs_orbit_f64_bad> packed_bad;
    std::vector<fs_orbit_f32_bad> packed_f32_bad;
    std::vector<std::vector<fs_bla_f64>> levels;
    std::vector<const void *> ptrs;
    std::vector<uint64_t> sizes;
    int32_t lm2 = 0;
};

// ------------------------------------------------------------------ Feature Finder scan (feature_scan.cpp)
enum FeatStage { kFind = 0, kNewton = 1, kFinal1 = 2, kFinal2 = 3, kFound = 4, kRejected = 5 };

template <class F> struct FeatCand {
    Mp cx, cy;
    uint32_t grid = 0;
    int stage = kFind;
    uint32_t it = 0;
    uint64_t period = 0;
    hreal<double> residual2{};
    Mp radius;
};

struct fsh_feature {
    int is64 = 0; // T is 64 bits wide: the candidates are in c64, else in c32
    int kind = 0; // T: 0 HDRFloat<float>, 1 HDRFloat<double>, 2 float, 3 double
    uint32_t iter_bytes = 4;
    uint64_t max_iters = 0;
    uint64_t prec_bits = 0;
    bool direct = false; // Direct / DirectScan: no orbit, records carry an all-zero dc
    Mp hiX, hiY;     // the reference orbit's point (results.GetHiX / GetHiY)
    Mp radius_hp;    // FeatureSummary radius: half the view's height / 12
    std::vector<FeatCand<float>> c32;
    std::vector<FeatCand<double>> c64;
    std::vector<uint32_t> batch; // candidates of the last batch, in record order
};
