// plain_inputs.cpp -- inputs in plain float / double: orbit + LAv2 table (fsh_plain), and the double orbit with its BLA table
// (fsh_orbit_f64).
#include "inputs_state.hpp"

// ------------------------------------------------------------------ plain float / double orbit + LAv2 table
// Inputs of Gpu1x32PerturbedLAv2* (T = float), Gpu1x64PerturbedLAv2* (T = double) and, converted field-wise,
// Gpu2x32PerturbedLAv2* (T = CudaDblflt<MattDblflt>, built as double: DoubleTo2x32Converter, Fractal.cpp:2771-2772).
// Orbit: the floatOrDouble arms of AddPerturbationReferencePointST (RefOrbitCalc.cpp:481-488,524-530,564-604,617-622)
// with T = float | double; table: LAReference<uint32_t,T,T,Disable> through the builder of la_table.cpp with F = plain<T>.
namespace {
// compression_exp >= 0: PerturbExtras::SimpleCompression through RefOrbitCompressor<IterType, T, SimpleCompression>
// (PerturbationResults.cpp:2334-2381) in plain T arithmetic.
template <class T>
void build_plain_orbit(const fsh_view &vw, uint64_t max_iter, int periodicity, PlainOrbit<T> &ob, int compression_exp = -1)
{
    mpf_set_default_prec(vw.prec_bits);
    {
        Mp two = Mp::from_ui(2);
        ob.cx = (vw.maxX + vw.minX) / two;
        ob.cy = (vw.maxY + vw.minY) / two;
        Mp delta = vw.maxY - vw.minY;
        ob.maxRadius = preal<T>{(T)((T)mpf_get_d(delta.v) / T(2.0f))}; // T{delta} / T{2.0f}, PerturbationResults.cpp:823-824
    }
    ob.x.push_back(preal<T>{T(0)});
    ob.y.push_back(preal<T>{T(0)});
    ob.bad.assign(1, 0);
    MpStepper s(ob.cx, ob.cy);
    T dzdcX = T(1), dzdcY = T(0);
    const T cx_cast = (T)mpf_get_d(s.cx), cy_cast = (T)mpf_get_d(s.cy);
    ob.orbitXLow = cx_cast; // m_OrbitXLow = T{cx}, PerturbationResults.cpp:852-853
    ob.orbitYLow = cy_cast;
    ob.compressed = compression_exp >= 0;
    ob.wp_index.assign(1, 0);
    ob.wp_x.assign(1, T(0));
    ob.wp_y.assign(1, T(0));
    uint64_t count = 1; // m_UncompressedItersInOrbit
    T rc_zx = ob.orbitXLow, rc_zy = ob.orbitYLow;
    const T rc_err = static_cast<T>(std::pow(10, compression_exp));
    for (uint64_t i = 0; i < max_iter; i++) {
        const T double_zx = (T)mpf_get_d(s.zx), double_zy = (T)mpf_get_d(s.zy);
        if (!ob.compressed) {
            ob.x.push_back(preal<T>{double_zx});
            ob.y.push_back(preal<T>{double_zy});
        } else {
            // MaybeAddCompressedIteration({double_zx, double_zy, i + 1})
            const T errX = rc_zx - double_zx, errY = rc_zy - double_zy;
            const T norm_z = double_zx * double_zx + double_zy * double_zy;
            const T err = (errX * errX + errY * errY) * rc_err;
            if (err >= norm_z) {
                ob.wp_index.push_back(i + 1);
                ob.wp_x.push_back(double_zx);
                ob.wp_y.push_back(double_zy);
                rc_zx = double_zx;
                rc_zy = double_zy;
            }
            rc_one_iter_plain(rc_zx, rc_zy, ob.orbitXLow, ob.orbitYLow);
        }
        count++;
        {
            // PerturbExtras::Bad, RefOrbitCalc.cpp:550-562: entries whose parts or norm underflow a binary32 (in double)
            const double small_float = 1.1754944e-38, glitch = 0.0000001, bx = double_zx, by = double_zy;
            const double norm = (bx * bx + by * by) * glitch;
            ob.bad.push_back((std::fabs(bx) <= small_float || std::fabs(by) <= small_float || norm <= small_float) ? 1 : 0);
        }
        if (periodicity) {
            const T n2 = std::max(std::fabs(double_zx), std::fabs(double_zy));
            const T r0 = std::max(std::fabs(dzdcX), std::fabs(dzdcY));
            const T n3 = ob.maxRadius.m * r0 * T(2);
            if (n2 < n3) {
                ob.period = count;
                break;
            } else {
                const T dzdcXOrig = dzdcX;
                dzdcX = T(2) * (double_zx * dzdcX - double_zy * dzdcY) + T(1);
                dzdcY = T(2) * (double_zx * dzdcY + double_zy * dzdcXOrig);
            }
        }
        s.step();
        const T tempZX = double_zx + cx_cast, tempZY = double_zy + cy_cast;
        const T zn = tempZX * tempZX + tempZY * tempZY;
        if (zn > T(256))
            break;
    }
    ob.bad.back() = 0; // results->SetBad(false), RefOrbitCalc.cpp:625-627
    if (ob.compressed) {
        // the orbit every host consumer (the LA builder) sees: RuntimeDecompressor::GetCompressedComplex
        ob.x.assign(count, preal<T>{T(0)});
        ob.y.assign(count, preal<T>{T(0)});
        for (size_t k = 0; k < ob.wp_index.size(); k++) {
            const uint64_t i0 = ob.wp_index[k];
            const uint64_t i1 = k + 1 < ob.wp_index.size() ? ob.wp_index[k + 1] : count;
            T zx_ = ob.wp_x[k], zy_ = ob.wp_y[k];
            for (uint64_t i = i0; i < i1; i++) {
                ob.x[i] = preal<T>{zx_};
                ob.y[i] = preal<T>{zy_};
                rc_one_iter_plain(zx_, zy_, ob.orbitXLow, ob.orbitYLow);
            }
        }
    }
}
} // namespace

template <class T>
void PlainInputs<T>::build(const fsh_view &vw, uint64_t max_iter, int periodicity, int host_threads, int compression_exp)
{
    build_plain_orbit<T>(vw, max_iter, periodicity, ob, compression_exp);
    finish(host_threads);
}
// everything derived from the orbit (packed records, LA table, ATInfo): also what a loaded ".im" orbit goes through
template <class T> void PlainInputs<T>::finish(int host_threads)
{
    using R = plain_recs<T>;
    orbit_packed.resize(ob.x.size());
    for (size_t i = 0; i < ob.x.size(); i++)
        orbit_packed[i] = typename R::orbit{ob.x[i].m, ob.y[i].m};
    if (ob.compressed) {
        rc_packed.resize(ob.wp_index.size());
        for (size_t k = 0; k < ob.wp_index.size(); k++)
            rc_packed[k] = typename R::orbit_rc{ob.wp_index[k], ob.wp_x[k], ob.wp_y[k]};
    }
    la_generate<plain<T>>(ob, t, host_threads < 1 ? 1 : host_threads);
    auto C = [](pcplx<T> c) { return typename R::cplx{c.re, c.im}; };
    la_packed.resize(t.las.size());
    for (size_t k = 0; k < t.las.size(); k++) {
        const auto &s = t.las[k];
        typename R::la r;
        memset(&r, 0, sizeof(r));
        r.Ref = C(s.Ref);
        r.ZCoeff = C(s.ZCoeff);
        r.CCoeff = C(s.CCoeff);
        r.LAThreshold = s.LAThreshold.m;
        r.LAThresholdC = s.LAThresholdC.m;
        r.MinMag = s.MinMag.m;
        r.StepLength = s.StepLength;
        r.NextStageLAIndex = s.NextStageLAIndex;
        la_packed[k] = r;
    }
    const auto &a = t.at;
    memset(&at_packed, 0, sizeof(at_packed));
    at_packed.StepLength = a.StepLength;
    at_packed.ThresholdC = a.ThresholdC.m;
    at_packed.SqrEscapeRadius = a.SqrEscapeRadius.m;
    at_packed.RefC = C(a.RefC);
    at_packed.ZCoeff = C(a.ZCoeff);
    at_packed.CCoeff = C(a.CCoeff);
    at_packed.InvZCoeff = C(a.InvZCoeff);
    at_packed.CCoeffSqrInvZCoeff = C(a.CCoeffSqrInvZCoeff);
    at_packed.CCoeffInvZCoeff = C(a.CCoeffInvZCoeff);
    at_packed.CCoeffNormSqr = a.CCoeffNormSqr.m;
    at_packed.RefCNormSqr = a.RefCNormSqr.m;
    at_packed.factor = a.factor.m;
}
template struct PlainInputs<float>;
template struct PlainInputs<double>;

extern "C" fsh_plain *fsh_plain_create_ex(const fsh_view *v, int kind, uint64_t max_iter, int periodicity, int host_threads,
                                          int compression_exp)
{
    if (kind != 0 && kind != 1)
        return nullptr;
    auto h = std::make_unique<fsh_plain>();
    h->kind = kind;
    if (kind == 0)
        h->f.build(*v, max_iter, periodicity, host_threads, compression_exp);
    else
        h->d.build(*v, max_iter, periodicity, host_threads, compression_exp);
    return h.release();
}
extern "C" fsh_plain *fsh_plain_create(const fsh_view *v, int kind, uint64_t max_iter, int periodicity, int host_threads)
{
    return fsh_plain_create_ex(v, kind, max_iter, periodicity, host_threads, -1);
}
extern "C" void fsh_plain_destroy(fsh_plain *h) { delete h; }
extern "C" int fsh_plain_kind(const fsh_plain *h) { return h->kind; }
#define FS_PLAIN_GET(EXPR_F, EXPR_D) (h->kind == 0 ? (EXPR_F) : (EXPR_D))
extern "C" uint64_t fsh_plain_orbit_count(const fsh_plain *h) { return FS_PLAIN_GET(h->f.ob.x.size(), h->d.ob.x.size()); }
extern "C" uint64_t fsh_plain_orbit_period(const fsh_plain *h) { return FS_PLAIN_GET(h->f.ob.period, h->d.ob.period); }
extern "C" const void *fsh_plain_orbit_data(const fsh_plain *h)
{
    return FS_PLAIN_GET((const void *)h->f.orbit_packed.data(), (const void *)h->d.orbit_packed.data());
}
extern "C" int fsh_plain_is_compressed(const fsh_plain *h) { return FS_PLAIN_GET(h->f.ob.compressed, h->d.ob.compressed) ? 1 : 0; }
extern "C" uint64_t fsh_plain_compressed_count(const fsh_plain *h)
{
    return FS_PLAIN_GET(h->f.rc_packed.size(), h->d.rc_packed.size());
}
extern "C" const void *fsh_plain_compressed_data(const fsh_plain *h)
{
    return FS_PLAIN_GET((const void *)h->f.rc_packed.data(), (const void *)h->d.rc_packed.data());
}
extern "C" void fsh_plain_orbit_low(const fsh_plain *h, void *out)
{
    if (h->kind == 0) {
        ((float *)out)[0] = h->f.ob.orbitXLow;
        ((float *)out)[1] = h->f.ob.orbitYLow;
    } else {
        ((double *)out)[0] = h->d.ob.orbitXLow;
        ((double *)out)[1] = h->d.ob.orbitYLow;
    }
}
extern "C" uint32_t fsh_plain_la_count(const fsh_plain *h)
{
    return (uint32_t)FS_PLAIN_GET(h->f.la_packed.size(), h->d.la_packed.size());
}
extern "C" const void *fsh_plain_la_data(const fsh_plain *h)
{
    return FS_PLAIN_GET((const void *)h->f.la_packed.data(), (const void *)h->d.la_packed.data());
}
extern "C" uint32_t fsh_plain_la_stage_count(const fsh_plain *h) { return FS_PLAIN_GET(h->f.t.stageCount, h->d.t.stageCount); }
extern "C" const fs_la_stage_u32 *fsh_plain_la_stages(const fsh_plain *h)
{
    return FS_PLAIN_GET(h->f.t.packedStages.data(), h->d.t.packedStages.data());
}
extern "C" int fsh_plain_la_is_valid(const fsh_plain *h) { return FS_PLAIN_GET(h->f.t.isValid, h->d.t.isValid) ? 1 : 0; }
extern "C" int fsh_plain_la_use_at(const fsh_plain *h) { return FS_PLAIN_GET(h->f.t.useAT, h->d.t.useAT) ? 1 : 0; }
extern "C" void fsh_plain_la_at(const fsh_plain *h, void *out)
{
    if (h->kind == 0)
        memcpy(out, &h->f.at_packed, sizeof(h->f.at_packed));
    else
        memcpy(out, &h->d.at_packed, sizeof(h->d.at_packed));
}
#undef FS_PLAIN_GET
// {dx, dy, centerX, centerY} (FillGpuCoords / FillCoord, Fractal.cpp:1782-1786,1813-1817,1833-1844, :2828-2832):
// float[4] for kind 0, double[4] for kind 1.
extern "C" void fsh_plain_coords(const fsh_view *v, const fsh_plain *h, uint32_t w_aa, uint32_t h_aa, void *out)
{
    mpf_set_default_prec(v->prec_bits);
    Mp dx = (v->maxX - v->minX) / Mp::from_ui(w_aa);
    Mp dy = (v->maxY - v->minY) / Mp::from_ui(h_aa);
    const Mp &ocx = h->kind == 0 ? h->f.ob.cx : h->d.ob.cx;
    const Mp &ocy = h->kind == 0 ? h->f.ob.cy : h->d.ob.cy;
    Mp cX = ocx - v->minX;
    Mp cY = ocy - v->maxY;
    const double d[4] = {mpf_get_d(dx.v), mpf_get_d(dy.v), mpf_get_d(cX.v), mpf_get_d(cY.v)};
    for (int i = 0; i < 4; i++) {
        if (h->kind == 0)
            ((float *)out)[i] = (float)d[i];
        else
            ((double *)out)[i] = d[i];
    }
}

// ------------------------------------------------------------------ plain double (Cpu64PerturbedBLA / Gpu1x64PerturbedBLA)
// PerturbationResults<uint32_t,double,Disable> + BLAS<uint32_t,double>: the floatOrDouble branches of
// AddPerturbationReferencePointST (RefOrbitCalc.cpp:481-488,524-530,564-604,617-622) and BLAS.cpp with T = double.
extern "C" fsh_orbit_f64 *fsh_orbit_f64_create(const fsh_view *v, uint64_t max_iter, int periodicity)
{
    auto o = std::make_unique<fsh_orbit_f64>();
    const PlainOrbit<double> &ob = o->ob;
    build_plain_orbit<double>(*v, max_iter, periodicity, o->ob);
    o->z.resize(ob.x.size());
    for (size_t i = 0; i < ob.x.size(); i++)
        o->z[i] = fs_orbit_f64{ob.x[i].m, ob.y[i].m};
    // BLAS<uint32_t,double>::Init(count, maxRadius), BLAS.cpp:25-255 with plain double (BLA.cuh:40-91)
    const auto &Z = o->z;
    const double blaSize = ob.maxRadius.m;
    const double epsilon = 1.0 / 8388608.0; // T(1) / T{1L << 23}
    auto one_step = [&](size_t mm) {
        const double RealA = Z[mm].x * 2, ImagA = Z[mm].y * 2;
        const double mA = std::sqrt(RealA * RealA + ImagA * ImagA);
        const double r = mA * epsilon;
        return fs_bla_f64{r * r, RealA, ImagA, 1.0, 0.0, 1, 0};
    };
    auto merge = [&](const fs_bla_f64 &x, const fs_bla_f64 &y) {
        const int32_t l = x.l + y.l;
        const double RealA = y.Ax * x.Ax - y.Ay * x.Ay;
        const double ImagA = y.Ax * x.Ay + y.Ay * x.Ax;
        const double RealB = y.Ax * x.Bx - y.Ay * x.By + y.Bx;
        const double ImagB = y.Ax * x.By + y.Ay * x.Bx + y.By;
        const double xA = std::sqrt(x.Ax * x.Ax + x.Ay * x.Ay);
        const double xB = std::sqrt(x.Bx * x.Bx + x.By * x.By);
        const double tempR = (std::sqrt(y.r2) - xB * blaSize) / xA;
        const double mx = (0.0 > tempR) ? 0.0 : tempR;           // HdrMaxReduced(T(0), tempR)
        const double sx = std::sqrt(x.r2);
        const double r = (sx < mx) ? sx : mx;                    // HdrMinPositiveReduced
        return fs_bla_f64{r * r, RealA, ImagA, RealB, ImagB, l, 0};
    };
    o->lm2 = bla_pyramid(Z.size(), o->levels, one_step, merge);
    bla_export(o->levels, o->ptrs, o->sizes);
    return o.release();
}
// PerturbExtras::Bad form of the double orbit + its binary32 copy (Gpu1x32PerturbedScaled)
extern "C" const fs_orbit_f64_bad *fsh_orbit_f64_data_bad(fsh_orbit_f64 *o)
{
    if (o->packed_bad.size() != o->z.size()) {
        o->packed_bad.resize(o->z.size());
        for (size_t i = 0; i < o->z.size(); i++)
            o->packed_bad[i] = fs_orbit_f64_bad{o->ob.bad[i], 0u, o->z[i].x, o->z[i].y};
    }
    return o->packed_bad.data();
}
extern "C" const fs_orbit_f32_bad *fsh_orbit_f64_data_f32_bad(fsh_orbit_f64 *o)
{
    if (o->packed_f32_bad.size() != o->z.size()) {
        o->packed_f32_bad.resize(o->z.size());
        for (size_t i = 0; i < o->z.size(); i++)
            o->packed_f32_bad[i] = fs_orbit_f32_bad{o->ob.bad[i] != 0 ? 1u : 0u, 0u, (float)o->z[i].x, (float)o->z[i].y};
    }
    return o->packed_f32_bad.data();
}

extern "C" void fsh_orbit_f64_destroy(fsh_orbit_f64 *o) { delete o; }
extern "C" uint64_t fsh_orbit_f64_count(const fsh_orbit_f64 *o) { return o->z.size(); }
extern "C" uint64_t fsh_orbit_f64_period(const fsh_orbit_f64 *o) { return o->ob.period; }
extern "C" const fs_orbit_f64 *fsh_orbit_f64_data(const fsh_orbit_f64 *o) { return o->z.data(); }
extern "C" int32_t fsh_orbit_f64_bla_num_levels(const fsh_orbit_f64 *o) { return (int32_t)o->ptrs.size(); }
extern "C" int32_t fsh_orbit_f64_bla_lm2(const fsh_orbit_f64 *o) { return o->lm2; }
extern "C" const void *const *fsh_orbit_f64_bla_level_ptrs(const fsh_orbit_f64 *o) { return o->ptrs.data(); }
extern "C" const uint64_t *fsh_orbit_f64_bla_level_sizes(const fsh_orbit_f64 *o) { return o->sizes.data(); }
// {dx, dy, centerX, centerY} as doubles (Fractal.cpp:2230-2238 with T = double: mpf_get_d, no reduction).
extern "C" void fsh_view_coords_perturb_f64(const fsh_view *v, const fsh_orbit_f64 *o, uint32_t w_aa, uint32_t h_aa,
                                            double out[4])
{
    mpf_set_default_prec(v->prec_bits);
    Mp dx = (v->maxX - v->minX) / Mp::from_ui(w_aa);
    Mp dy = (v->maxY - v->minY) / Mp::from_ui(h_aa);
    Mp cX = o->ob.cx - v->minX;
    Mp cY = o->ob.cy - v->maxY;
    out[0] = mpf_get_d(dx.v);
    out[1] = mpf_get_d(dy.v);
    out[2] = mpf_get_d(cX.v);
    out[3] = mpf_get_d(cY.v);
}
