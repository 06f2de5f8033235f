// feature_scan.cpp -- Feature Finder scan (fsh_feature_*).
#include "inputs_state.hpp"

// FeatureFinderOrchestrator's PT / PTScan grid (FeatureFinderOrchestrator.cpp:485-559) and FeatureFinder::FindPeriodicPoint_Common
// up to SetFound (FeatureFinder.cpp:2443-2697), restated as a batched state machine: every candidate's evaluations are asked for
// together (fsh_feature_next_batch), made elsewhere (fs_feature_eval or the CPU checker), and handed back (fsh_feature_consume);
// the Newton updates stay here, in mpf, as the reference keeps them.  FeatureFinder::Params defaults (FeatureFinder.h:58-63):
// MaxNewtonIters 32, RelStepTol 2^-40, Eps2Accept = T{} (off).  The Direct / DirectScan modes (fsh_feature_begin_direct*) are the same
// machine without an orbit: FindPeriodicPoint_Common takes nothing from it, only PTEvaluator does (dc), so their records carry dc = 0.
namespace {

// HighPrecision{HDRFloat<F>} (HDRFloat.h:396-411): exact, at 64 bits.
template <class F> Mp mp_from_hr(hreal<F> v)
{
    Mp r(64, 0);
    mpf_set_d(r.v, (double)v.m);
    if (v.e >= 0)
        mpf_mul_2exp(r.v, r.v, (mp_bitcnt_t)v.e);
    else
        mpf_div_2exp(r.v, r.v, (mp_bitcnt_t)(-(int64_t)v.e));
    return r;
}

template <class F> hcplx<F> ct_from_mp(const Mp &x, const Mp &y)
{
    return hc_reduced(hc_from_hr(hr_from_mpf<F>(x.v), hr_from_mpf<F>(y.v)));
}

// FeatureFinder::Div (FeatureFinder.cpp:1550-1574), in HDRFloat<double>.
template <class F> hcplx<F> feat_div(hcplx<F> a, hcplx<F> b)
{
    using H = hreal<double>;
    const H br{(double)b.re, b.e}, bi{(double)b.im, b.e};
    const H denom = hr_reduced(hr_add(hr_mul(br, br), hr_mul(bi, bi)));
    if (hr_cmp_pos(denom, hr_zero<double>()) <= 0)
        return hc_zero<F>();
    const H ar{(double)a.re, a.e}, ai{(double)a.im, a.e};
    const H rr = hr_reduced(hr_div(hr_add(hr_mul(ar, br), hr_mul(ai, bi)), denom));
    const H ii = hr_reduced(hr_div(hr_sub(hr_mul(ai, br), hr_mul(ar, bi)), denom));
    return hc_from_hr(hreal<F>{(F)rr.m, rr.e}, hreal<F>{(F)ii.m, ii.e});
}

template <class F> hreal<F> ld_real(const void *p)
{
    if constexpr (sizeof(F) == 4) {
        const fs_real_hdr32 *r = (const fs_real_hdr32 *)p;
        return hreal<F>{r->m, r->e};
    } else {
        const fs_real_hdr64 *r = (const fs_real_hdr64 *)p;
        return hreal<F>{r->m, r->e};
    }
}

template <class F> std::vector<FeatCand<F>> &cands(fsh_feature &f);
template <> std::vector<FeatCand<float>> &cands<float>(fsh_feature &f) { return f.c32; }
template <> std::vector<FeatCand<double>> &cands<double>(fsh_feature &f) { return f.c64; }

// PointZoomBBConverter::X/YFromScreenToCalc (PointZoomBBConverter.cpp:339-354), antialiasing 1
struct FeatScreen {
    uint64_t prec;
    Mp wX, wY, OriginX, OriginY, hwaa, hhaa;
    explicit FeatScreen(const fsh_view &v)
        : prec(v.prec_bits), wX(v.maxX - v.minX), wY(v.maxY - v.minY), OriginX(v.prec_bits, 0), OriginY(v.prec_bits, 0),
          hwaa(v.prec_bits, 0), hhaa(v.prec_bits, 0)
    {
        const Mp aa = Mp::from_ui(1), highWidth = Mp::from_ui(v.width), highHeight = Mp::from_ui(v.height);
        Mp negMinX(v.minX.prec(), 0);
        mpf_neg(negMinX.v, v.minX.v);
        mpf_mul(hwaa.v, highWidth.v, aa.v);
        mpf_div(OriginX.v, hwaa.v, wX.v);
        mpf_mul(OriginX.v, OriginX.v, negMinX.v);
        mpf_mul(hhaa.v, highHeight.v, aa.v);
        mpf_div(OriginY.v, hhaa.v, wY.v);
        mpf_mul(OriginY.v, OriginY.v, v.maxY.v);
    }
    Mp X(uint64_t x) const
    {
        Mp px = Mp::from_ui(x), cx(prec, 0);
        mpf_sub(cx.v, px.v, OriginX.v);
        mpf_mul(cx.v, cx.v, wX.v);
        mpf_div(cx.v, cx.v, hwaa.v);
        return cx;
    }
    Mp Y(uint64_t y) const
    {
        Mp py = Mp::from_ui(y), cy(prec, 0);
        mpf_sub(cy.v, py.v, OriginY.v);
        mpf_neg(cy.v, cy.v);
        mpf_mul(cy.v, cy.v, wY.v);
        mpf_div(cy.v, cy.v, hhaa.v);
        return cy;
    }
};

// The scan's screen points (FeatureFinderOrchestrator.cpp:541-548)
inline uint64_t feat_grid_px(uint64_t extent, uint32_t g, uint32_t n) { return (extent * (2 * (uint64_t)g + 1)) / (2 * (uint64_t)n); }

// The candidates: `at` = the one screen point of the non-scan mode instead of the nx x ny grid.  F picks the list only.
template <class F> void feature_grid(fsh_feature &f, const fsh_view &v, uint32_t nx, uint32_t ny, const uint64_t *at)
{
    const FeatScreen scr(v);
    auto &cs = cands<F>(f);
    auto add = [&](uint64_t x, uint64_t y, uint32_t grid) {
        FeatCand<F> c;
        c.cx = scr.X(x);
        c.cy = scr.Y(y);
        c.grid = grid;
        cs.push_back(c);
    };
    if (at) {
        add(at[0], at[1], 0);
        return;
    }
    for (uint32_t gy = 0; gy < ny; ++gy)
        for (uint32_t gx = 0; gx < nx; ++gx)
            add(feat_grid_px(v.width, gx, nx), feat_grid_px(v.height, gy, ny), gy * nx + gx);
}

template <class F>
void feature_begin(fsh_feature &f, const fsh_view &v, uint32_t nx, uint32_t ny, const uint64_t *at = nullptr)
{
    mpf_set_default_prec(v.prec_bits);
    // radiusY = T{MaxY - MinY} / T{2.0f}; HighPrecision radius{radiusY}; radius /= HighPrecision{12}
    const hreal<F> radiusY = hr_div(hr_from_mpf<F>((v.maxY - v.minY).v), hr_from_number<F>(F(2)));
    f.radius_hp = mp_from_hr(radiusY);
    {
        Mp twelve = Mp::from_ui(12);
        mpf_div(f.radius_hp.v, f.radius_hp.v, twelve.v);
    }
    feature_grid<F>(f, v, nx, ny, at);
}

// FindPeriodicPoint_Common's search radius: R = HdrAbs(T{radius}), SqrRadius = R * R reduced; what PTEvaluator::Eval passes on
// is HdrSqrt(SqrRadius).
template <class F> hreal<F> feature_eval_radius(const fsh_feature &f)
{
    hreal<F> R = hr_abs(hr_from_mpf<F>(f.radius_hp.v));
    const hreal<F> sqr = hr_reduced(hr_mul(R, R));
    return hr_sqrt(sqr);
}

template <class F, class In> uint64_t feature_next(fsh_feature &f, In *in, uint64_t cap, int *mode)
{
    auto &cs = cands<F>(f);
    f.batch.clear();
    // one mode per batch: while any candidate still waits for its period search, a batch holds only those
    bool any_find = false;
    for (const FeatCand<F> &c : cs)
        any_find |= c.stage == kFind;
    for (uint32_t k = 0; k < cs.size(); ++k)
        if (cs[k].stage < kFound && (cs[k].stage == kFind) == any_find && f.batch.size() < cap) {
            FeatCand<F> &c = cs[k];
            const hcplx<F> cc = ct_from_mp<F>(c.cx, c.cy);
            In r{};
            if (!f.direct) {
                const hcplx<F> dc = ct_from_mp<F>(c.cx - f.hiX, c.cy - f.hiY);
                r.dc.re = dc.re, r.dc.im = dc.im, r.dc.e = dc.e;
            }
            r.c.re = cc.re, r.c.im = cc.im, r.c.e = cc.e;
            r.period = c.stage == kFind ? 0 : c.period;
            in[f.batch.size()] = r;
            f.batch.push_back(k);
        }
    *mode = any_find ? 0 : 1;
    return f.batch.size();
}

// The Newton step of FindPeriodicPoint_Common: c <- c - diff / dzdc, in mpf only.  False: dzdc is degenerate (rejected).
template <class F> bool newton_step(FeatCand<F> &c, hcplx<F> diff, hcplx<F> dzdc, hcplx<F> *step_out)
{
    if (hr_cmp_pos(hr_reduced(hc_norm2(dzdc)), hr_zero<F>()) <= 0)
        return false;
    const hcplx<F> step = hc_reduced(feat_div(diff, dzdc));
    c.cx = c.cx - mp_from_hr(hc_re(step));
    c.cy = c.cy - mp_from_hr(hc_im(step));
    if (step_out)
        *step_out = step;
    return true;
}

template <class F, class Out> void feature_consume(fsh_feature &f, const Out *out, uint64_t n)
{
    auto &cs = cands<F>(f);
    const hreal<F> tol = hr_reduced(hr_from_number<F>(F(0x1p-40))); // diffTol and RelStepTol alike
    const hreal<F> tol2 = hr_reduced(hr_mul(tol, tol));
    for (uint64_t j = 0; j < n && j < f.batch.size(); ++j) {
        FeatCand<F> &c = cs[f.batch[j]];
        const Out &o = out[j];
        if (o.status == 0) { // rejected: findPeriod / evalAtPeriod / final eval failed
            c.stage = kRejected;
            continue;
        }
        const hcplx<F> diff{o.diff.re, o.diff.im, o.diff.e}, dzdc{o.dzdc.re, o.dzdc.im, o.dzdc.e};
        const hcplx<F> zcoeff{o.zcoeff.re, o.zcoeff.im, o.zcoeff.e};
        switch (c.stage) {
        case kFind:
            c.period = o.period;
            c.stage = newton_step<F>(c, diff, dzdc, nullptr) ? kNewton : kRejected;
            break;
        case kNewton: {
            const hcplx<F> cT = ct_from_mp<F>(c.cx, c.cy);
            const hreal<F> diff2 = hr_reduced(hc_norm2(diff));
            if (hr_cmp_pos(diff2, hr_reduced(hr_mul(hr_reduced(hc_norm2(cT)), tol2))) <= 0) {
                c.stage = kFinal1;
                break;
            }
            hcplx<F> step;
            if (!newton_step<F>(c, diff, dzdc, &step)) {
                c.stage = kRejected;
                break;
            }
            const hcplx<F> cNew = ct_from_mp<F>(c.cx, c.cy);
            const hreal<F> step2 = hr_reduced(hc_norm2(step));
            if (hr_cmp_pos(step2, hr_reduced(hr_mul(hr_reduced(hc_norm2(cNew)), tol2))) <= 0 || ++c.it >= 32)
                c.stage = kFinal1;
            break;
        }
        case kFinal1:
            c.stage = newton_step<F>(c, diff, dzdc, nullptr) ? kFinal2 : kRejected;
            break;
        case kFinal2: {
            // the candidate store's w test (:2636-2662), then ComputeIntrinsicRadius_HP (:1713-1746)
            using H = hreal<double>;
            const H zr{(double)zcoeff.re, zcoeff.e}, zi{(double)zcoeff.im, zcoeff.e};
            const H dr{(double)dzdc.re, dzdc.e}, di{(double)dzdc.im, dzdc.e};
            const H wr = hr_reduced(hr_sub(hr_mul(zr, dr), hr_mul(zi, di)));
            const H wi = hr_reduced(hr_add(hr_mul(zr, di), hr_mul(zi, dr)));
            const H w2 = hr_reduced(hr_add(hr_mul(wr, wr), hr_mul(wi, wi)));
            if (!(hr_cmp_pos(w2, hr_zero<double>()) > 0)) {
                c.stage = kRejected;
                break;
            }
            const H absW = hr_reduced(hr_sqrt(w2));
            const H radius = hr_reduced(hr_div(hr_from_number<double>(4.0), absW));
            c.radius = mp_from_hr(radius);
            const hreal<F> r2{o.residual2.m, o.residual2.e};
            c.residual2 = H{(double)r2.m, r2.e};
            c.stage = kFound;
            break;
        }
        default:
            break;
        }
    }
}

template <class F> const FeatCand<F> *found_at(fsh_feature &f, uint64_t k)
{
    uint64_t seen = 0;
    for (const FeatCand<F> &c : cands<F>(f))
        if (c.stage == kFound && seen++ == k)
            return &c;
    return nullptr;
}

} // namespace

extern "C" fsh_feature *fsh_feature_begin(const fsh_view *v, const fsh_orbit *o, uint32_t nx, uint32_t ny, uint32_t iter_bytes,
                                          uint64_t max_iters)
{
    if (!v || !o || nx == 0 || ny == 0 || (iter_bytes != 4 && iter_bytes != 8))
        return nullptr;
    auto f = std::make_unique<fsh_feature>();
    f->is64 = o->is64;
    f->kind = o->is64 ? 1 : 0;
    f->iter_bytes = iter_bytes;
    f->max_iters = max_iters;
    f->prec_bits = v->prec_bits;
    f->hiX = o->is64 ? o->d.cx : o->f.cx;
    f->hiY = o->is64 ? o->d.cy : o->f.cy;
    if (f->is64)
        feature_begin<double>(*f, *v, nx, ny);
    else
        feature_begin<float>(*f, *v, nx, ny);
    return f.release();
}

static fsh_feature *feature_begin_direct(const fsh_view *v, int is64, uint32_t nx, uint32_t ny, const uint64_t *at,
                                         uint32_t iter_bytes, uint64_t max_iters)
{
    if (!v || nx == 0 || ny == 0 || (iter_bytes != 4 && iter_bytes != 8))
        return nullptr;
    auto f = std::make_unique<fsh_feature>();
    f->is64 = is64 != 0;
    f->kind = f->is64;
    f->iter_bytes = iter_bytes;
    f->max_iters = max_iters;
    f->prec_bits = v->prec_bits;
    f->direct = true;
    if (f->is64)
        feature_begin<double>(*f, *v, nx, ny, at);
    else
        feature_begin<float>(*f, *v, nx, ny, at);
    return f.release();
}

extern "C" fsh_feature *fsh_feature_begin_direct(const fsh_view *v, int is64, uint32_t nx, uint32_t ny, uint32_t iter_bytes,
                                                 uint64_t max_iters)
{
    return feature_begin_direct(v, is64, nx, ny, nullptr, iter_bytes, max_iters);
}

extern "C" fsh_feature *fsh_feature_begin_direct_at(const fsh_view *v, int is64, uint32_t px, uint32_t py, uint32_t iter_bytes,
                                                    uint64_t max_iters)
{
    const uint64_t at[2] = {px, py};
    return feature_begin_direct(v, is64, 1, 1, at, iter_bytes, max_iters);
}

namespace {

template <class F, class In, class Real> void feature_direct_grid(const fsh_view &v, uint32_t nx, uint32_t ny, In *in, Real *radius)
{
    mpf_set_default_prec(v.prec_bits);
    fsh_feature f; // for its search radius only
    f.prec_bits = v.prec_bits;
    feature_begin<F>(f, v, 1, 1);
    const hreal<F> R = feature_eval_radius<F>(f);
    Real rad{};
    rad.m = R.m, rad.e = R.e;
    *radius = rad;
    // T{cX_hp} per column and T{cY_hp} per row; MakeCTFromHP = C(re, im), reduced, per point
    const FeatScreen scr(v);
    std::vector<hreal<F>> re(nx), im(ny);
    for (uint32_t gx = 0; gx < nx; ++gx)
        re[gx] = hr_from_mpf<F>(scr.X(feat_grid_px(v.width, gx, nx)).v);
    for (uint32_t gy = 0; gy < ny; ++gy)
        im[gy] = hr_from_mpf<F>(scr.Y(feat_grid_px(v.height, gy, ny)).v);
    for (uint32_t gy = 0; gy < ny; ++gy)
        for (uint32_t gx = 0; gx < nx; ++gx) {
            const hcplx<F> cc = hc_reduced(hc_from_hr(re[gx], im[gy]));
            In r{};
            r.c.re = cc.re, r.c.im = cc.im, r.c.e = cc.e;
            in[(size_t)gy * nx + gx] = r;
        }
}

} // namespace

extern "C" int fsh_feature_direct_grid(const fsh_view *v, int is64, uint32_t nx, uint32_t ny, void *in, void *radius)
{
    if (!v || nx == 0 || ny == 0 || !in || !radius)
        return -1;
    if (is64)
        feature_direct_grid<double>(*v, nx, ny, (fs_feature_in_hdr64 *)in, (fs_real_hdr64 *)radius);
    else
        feature_direct_grid<float>(*v, nx, ny, (fs_feature_in_hdr32 *)in, (fs_real_hdr32 *)radius);
    return 0;
}

namespace {

// The PT scan's find round over the grid, taken apart: feature_next's dc = ct_from_mp(cx - HiX, cy - HiY) and c = ct_from_mp(cx, cy)
// read cx of the column and cy of the row only, so T{..} of the four is made once per column and once per row.
template <class F> struct PtAxes {
    std::vector<hreal<F>> dc_re, dc_im, c_re, c_im;
    hreal<F> R;
};

template <class F> PtAxes<F> feature_pt_axes(const fsh_view &v, const Mp &hiX, const Mp &hiY, uint32_t nx, uint32_t ny)
{
    mpf_set_default_prec(v.prec_bits);
    fsh_feature f; // for its search radius only
    f.prec_bits = v.prec_bits;
    feature_begin<F>(f, v, 1, 1);
    PtAxes<F> a;
    a.R = feature_eval_radius<F>(f);
    const FeatScreen scr(v);
    a.dc_re.resize(nx), a.c_re.resize(nx), a.dc_im.resize(ny), a.c_im.resize(ny);
    for (uint32_t gx = 0; gx < nx; ++gx) {
        const Mp cx = scr.X(feat_grid_px(v.width, gx, nx));
        a.c_re[gx] = hr_from_mpf<F>(cx.v);
        a.dc_re[gx] = hr_from_mpf<F>((cx - hiX).v);
    }
    for (uint32_t gy = 0; gy < ny; ++gy) {
        const Mp cy = scr.Y(feat_grid_px(v.height, gy, ny));
        a.c_im[gy] = hr_from_mpf<F>(cy.v);
        a.dc_im[gy] = hr_from_mpf<F>((cy - hiY).v);
    }
    return a;
}

template <class F, class Real> void store_axis(const std::vector<hreal<F>> &a, void *out)
{
    for (size_t k = 0; k < a.size(); ++k) {
        Real r{};
        r.m = a[k].m, r.e = a[k].e;
        ((Real *)out)[k] = r;
    }
}

template <class F, class Real>
void feature_pt_axes_out(const fsh_view &v, const Mp &hiX, const Mp &hiY, uint32_t nx, uint32_t ny, void *dc_re, void *dc_im,
                         void *c_re, void *c_im, void *radius)
{
    const PtAxes<F> a = feature_pt_axes<F>(v, hiX, hiY, nx, ny);
    store_axis<F, Real>(a.dc_re, dc_re);
    store_axis<F, Real>(a.dc_im, dc_im);
    store_axis<F, Real>(a.c_re, c_re);
    store_axis<F, Real>(a.c_im, c_im);
    store_axis<F, Real>({a.R}, radius);
}

template <class F, class In, class Real>
void feature_pt_grid(const fsh_view &v, const Mp &hiX, const Mp &hiY, uint32_t nx, uint32_t ny, In *in, void *radius)
{
    const PtAxes<F> a = feature_pt_axes<F>(v, hiX, hiY, nx, ny);
    store_axis<F, Real>({a.R}, radius);
    for (uint32_t gy = 0; gy < ny; ++gy)
        for (uint32_t gx = 0; gx < nx; ++gx) {
            const hcplx<F> dc = hc_reduced(hc_from_hr(a.dc_re[gx], a.dc_im[gy]));
            const hcplx<F> cc = hc_reduced(hc_from_hr(a.c_re[gx], a.c_im[gy]));
            In r{};
            r.dc.re = dc.re, r.dc.im = dc.im, r.dc.e = dc.e;
            r.c.re = cc.re, r.c.im = cc.im, r.c.e = cc.e;
            in[(size_t)gy * nx + gx] = r;
        }
}

} // namespace

extern "C" int fsh_feature_pt_axes(const fsh_view *v, const fsh_orbit *o, int is64, uint32_t nx, uint32_t ny, void *dc_re,
                                   void *dc_im, void *c_re, void *c_im, void *radius)
{
    if (!v || !o || nx == 0 || ny == 0 || !dc_re || !dc_im || !c_re || !c_im || !radius || (is64 != 0) != (o->is64 != 0))
        return -1;
    if (o->is64)
        feature_pt_axes_out<double, fs_real_hdr64>(*v, o->d.cx, o->d.cy, nx, ny, dc_re, dc_im, c_re, c_im, radius);
    else
        feature_pt_axes_out<float, fs_real_hdr32>(*v, o->f.cx, o->f.cy, nx, ny, dc_re, dc_im, c_re, c_im, radius);
    return 0;
}

extern "C" int fsh_feature_pt_grid(const fsh_view *v, const fsh_orbit *o, int is64, uint32_t nx, uint32_t ny, void *in, void *radius)
{
    if (!v || !o || nx == 0 || ny == 0 || !in || !radius || (is64 != 0) != (o->is64 != 0))
        return -1;
    if (o->is64)
        feature_pt_grid<double, fs_feature_in_hdr64, fs_real_hdr64>(*v, o->d.cx, o->d.cy, nx, ny, (fs_feature_in_hdr64 *)in, radius);
    else
        feature_pt_grid<float, fs_feature_in_hdr32, fs_real_hdr32>(*v, o->f.cx, o->f.cy, nx, ny, (fs_feature_in_hdr32 *)in, radius);
    return 0;
}

// ------------------------------------------------------------------ T = float / double (fsh_feature_begin_plain*)
// The same machine with the reference's plain T: C = FloatComplex<T>, HdrReduce empty, compares the plain operators,
// T{HighPrecision} = mpf_get_d (which truncates) and then the cast (HighPrecision.h:497-506), HighPrecision{T} = mpf_set_d at the
// default precision (:175-179).  R, SqrRadius = R * R and the tolerances are in T, so SqrRadius underflows to 0 in a view narrow
// enough (float: below about 1e-21; double: below about 1e-160) and every candidate is then rejected, as in the reference.  Div
// and the intrinsic radius go through HDRFloat<double> (PromoteToHdrD / DemoteToT, FeatureFinder.h:206-226).
namespace {

template <class T> T pt_from_mp(const Mp &x) { return (T)mpf_get_d(x.v); }

template <class T> struct pcplx {
    T re, im;
};
template <class T> T pc_norm2(pcplx<T> a) { return a.re * a.re + a.im * a.im; }

using HD = hreal<double>;
// PromoteToHdrD of an arithmetic value: HDRFloat<double>(double) = {mant, 0} reduced (HDRFloat.h:206-212)
template <class T> HD promote(T v) { return hr_from_mant<double>((double)v); }

// FeatureFinder::Div (FeatureFinder.cpp:1550-1574)
template <class T> pcplx<T> feat_div_plain(pcplx<T> a, pcplx<T> b)
{
    const HD br = promote(b.re), bi = promote(b.im);
    const HD denom = hr_reduced(hr_add(hr_mul(br, br), hr_mul(bi, bi)));
    if (hr_cmp_pos(denom, hr_zero<double>()) <= 0)
        return pcplx<T>{T(0), T(0)};
    const HD ar = promote(a.re), ai = promote(a.im);
    const HD rr = hr_reduced(hr_div(hr_add(hr_mul(ar, br), hr_mul(ai, bi)), denom));
    const HD ii = hr_reduced(hr_div(hr_sub(hr_mul(ai, br), hr_mul(ar, bi)), denom));
    return pcplx<T>{(T)hr_to_native<double>(rr), (T)hr_to_native<double>(ii)};
}

template <class T> void feature_begin_plain(fsh_feature &f, const fsh_view &v, uint32_t nx, uint32_t ny, const uint64_t *at = nullptr)
{
    mpf_set_default_prec(v.prec_bits);
    // radiusY = T{MaxY - MinY} / T{2.0f}; HighPrecision radius{radiusY}; radius /= HighPrecision{12}
    const T radiusY = pt_from_mp<T>(v.maxY - v.minY) / T(2.0f);
    f.radius_hp = Mp();
    mpf_set_d(f.radius_hp.v, (double)radiusY);
    {
        Mp twelve = Mp::from_ui(12);
        mpf_div(f.radius_hp.v, f.radius_hp.v, twelve.v);
    }
    feature_grid<T>(f, v, nx, ny, at);
}

// R = HdrAbs(T{radius}), SqrRadius = R * R; what the evaluators get is HdrSqrt(SqrRadius)
template <class T> T feature_eval_radius_plain(const fsh_feature &f)
{
    const T R = std::fabs(pt_from_mp<T>(f.radius_hp));
    const T sqr = R * R;
    return std::sqrt(sqr);
}

template <class T, class In> uint64_t feature_next_plain(fsh_feature &f, In *in, uint64_t cap, int *mode)
{
    auto &cs = cands<T>(f);
    f.batch.clear();
    bool any_find = false;
    for (const FeatCand<T> &c : cs)
        any_find |= c.stage == kFind;
    for (uint32_t k = 0; k < cs.size(); ++k)
        if (cs[k].stage < kFound && (cs[k].stage == kFind) == any_find && f.batch.size() < cap) {
            FeatCand<T> &c = cs[k];
            In r{};
            if (!f.direct) {
                r.dc[0] = pt_from_mp<T>(c.cx - f.hiX);
                r.dc[1] = pt_from_mp<T>(c.cy - f.hiY);
            }
            r.c[0] = pt_from_mp<T>(c.cx);
            r.c[1] = pt_from_mp<T>(c.cy);
            r.period = c.stage == kFind ? 0 : c.period;
            in[f.batch.size()] = r;
            f.batch.push_back(k);
        }
    *mode = any_find ? 0 : 1;
    return f.batch.size();
}

// c <- c - diff / dzdc, in mpf only.  False: dzdc is degenerate (rejected) -- or the step is not finite, which mpf_set_d cannot
// take (the reference's HighPrecision{T} would abort there).
template <class T> bool newton_step_plain(FeatCand<T> &c, pcplx<T> diff, pcplx<T> dzdc, pcplx<T> *step_out)
{
    if (pc_norm2(dzdc) <= T(0))
        return false;
    const pcplx<T> step = feat_div_plain(diff, dzdc);
    if (!std::isfinite(step.re) || !std::isfinite(step.im))
        return false;
    Mp sx, sy;
    mpf_set_d(sx.v, (double)step.re);
    mpf_set_d(sy.v, (double)step.im);
    c.cx = c.cx - sx;
    c.cy = c.cy - sy;
    if (step_out)
        *step_out = step;
    return true;
}

template <class T, class Out> void feature_consume_plain(fsh_feature &f, const Out *out, uint64_t n)
{
    auto &cs = cands<T>(f);
    const T tol = T(0x1p-40); // diffTol and RelStepTol alike
    const T tol2 = tol * tol;
    for (uint64_t j = 0; j < n && j < f.batch.size(); ++j) {
        FeatCand<T> &c = cs[f.batch[j]];
        const Out &o = out[j];
        if (o.status == 0) {
            c.stage = kRejected;
            continue;
        }
        const pcplx<T> diff{o.diff[0], o.diff[1]}, dzdc{o.dzdc[0], o.dzdc[1]}, zcoeff{o.zcoeff[0], o.zcoeff[1]};
        switch (c.stage) {
        case kFind:
            c.period = o.period;
            c.stage = newton_step_plain<T>(c, diff, dzdc, nullptr) ? kNewton : kRejected;
            break;
        case kNewton: {
            const pcplx<T> cT{pt_from_mp<T>(c.cx), pt_from_mp<T>(c.cy)};
            if (pc_norm2(diff) <= pc_norm2(cT) * tol2) {
                c.stage = kFinal1;
                break;
            }
            pcplx<T> step;
            if (!newton_step_plain<T>(c, diff, dzdc, &step)) {
                c.stage = kRejected;
                break;
            }
            const pcplx<T> cNew{pt_from_mp<T>(c.cx), pt_from_mp<T>(c.cy)};
            if (pc_norm2(step) <= pc_norm2(cNew) * tol2 || ++c.it >= 32)
                c.stage = kFinal1;
            break;
        }
        case kFinal1:
            c.stage = newton_step_plain<T>(c, diff, dzdc, nullptr) ? kFinal2 : kRejected;
            break;
        case kFinal2: {
            // the candidate store's w test (:2636-2662), then ComputeIntrinsicRadius_HP (:1713-1746)
            const HD zr = promote(zcoeff.re), zi = promote(zcoeff.im), dr = promote(dzdc.re), di = promote(dzdc.im);
            const HD wr = hr_reduced(hr_sub(hr_mul(zr, dr), hr_mul(zi, di)));
            const HD wi = hr_reduced(hr_add(hr_mul(zr, di), hr_mul(zi, dr)));
            const HD w2 = hr_reduced(hr_add(hr_mul(wr, wr), hr_mul(wi, wi)));
            if (!(hr_cmp_pos(w2, hr_zero<double>()) > 0)) {
                c.stage = kRejected;
                break;
            }
            const HD absW = hr_reduced(hr_sqrt(w2));
            const HD radius = hr_reduced(hr_div(hr_from_mant<double>(4.0), absW));
            c.radius = mp_from_hr(radius);
            // HDRFloat<double>{residual2}: of a float, the templated constructor (HDRFloat.h:295-317); of a double, {mant, 0}
            // reduced (:206-212) -- they differ for a zero only
            c.residual2 = sizeof(T) == 4 ? hr_from_number<double>((double)o.residual2) : hr_from_mant<double>((double)o.residual2);
            c.stage = kFound;
            break;
        }
        default:
            break;
        }
    }
}

fsh_feature *feature_begin_plain_any(const fsh_view *v, int kind, const Mp *hiX, const Mp *hiY, uint32_t nx, uint32_t ny,
                                     const uint64_t *at, uint32_t iter_bytes, uint64_t max_iters)
{
    if (!v || (kind != 0 && kind != 1) || nx == 0 || ny == 0 || (iter_bytes != 4 && iter_bytes != 8))
        return nullptr;
    auto f = std::make_unique<fsh_feature>();
    f->kind = 2 + kind;
    f->is64 = kind;
    f->iter_bytes = iter_bytes;
    f->max_iters = max_iters;
    f->prec_bits = v->prec_bits;
    f->direct = hiX == nullptr;
    if (hiX)
        f->hiX = *hiX, f->hiY = *hiY;
    if (kind)
        feature_begin_plain<double>(*f, *v, nx, ny, at);
    else
        feature_begin_plain<float>(*f, *v, nx, ny, at);
    return f.release();
}

} // namespace

extern "C" fsh_feature *fsh_feature_begin_plain(const fsh_view *v, const fsh_plain *p, uint32_t nx, uint32_t ny, uint32_t iter_bytes,
                                                uint64_t max_iters)
{
    if (!p)
        return nullptr;
    const Mp &hiX = p->kind == 0 ? p->f.ob.cx : p->d.ob.cx;
    const Mp &hiY = p->kind == 0 ? p->f.ob.cy : p->d.ob.cy;
    return feature_begin_plain_any(v, p->kind, &hiX, &hiY, nx, ny, nullptr, iter_bytes, max_iters);
}

extern "C" fsh_feature *fsh_feature_begin_plain_direct(const fsh_view *v, int kind, uint32_t nx, uint32_t ny, uint32_t iter_bytes,
                                                       uint64_t max_iters)
{
    return feature_begin_plain_any(v, kind, nullptr, nullptr, nx, ny, nullptr, iter_bytes, max_iters);
}

extern "C" fsh_feature *fsh_feature_begin_plain_direct_at(const fsh_view *v, int kind, uint32_t px, uint32_t py,
                                                          uint32_t iter_bytes, uint64_t max_iters)
{
    const uint64_t at[2] = {px, py};
    return feature_begin_plain_any(v, kind, nullptr, nullptr, 1, 1, at, iter_bytes, max_iters);
}

namespace {

template <class T, class In> void feature_plain_direct_grid(const fsh_view &v, uint32_t nx, uint32_t ny, In *in, T *radius)
{
    fsh_feature f; // for its search radius only
    f.prec_bits = v.prec_bits;
    feature_begin_plain<T>(f, v, 1, 1);
    *radius = feature_eval_radius_plain<T>(f);
    // T{cX_hp} per column and T{cY_hp} per row
    const FeatScreen scr(v);
    std::vector<T> re(nx), im(ny);
    for (uint32_t gx = 0; gx < nx; ++gx)
        re[gx] = pt_from_mp<T>(scr.X(feat_grid_px(v.width, gx, nx)));
    for (uint32_t gy = 0; gy < ny; ++gy)
        im[gy] = pt_from_mp<T>(scr.Y(feat_grid_px(v.height, gy, ny)));
    for (uint32_t gy = 0; gy < ny; ++gy)
        for (uint32_t gx = 0; gx < nx; ++gx) {
            In r{};
            r.c[0] = re[gx], r.c[1] = im[gy];
            in[(size_t)gy * nx + gx] = r;
        }
}

} // namespace

extern "C" int fsh_feature_plain_direct_grid(const fsh_view *v, int kind, uint32_t nx, uint32_t ny, void *in, void *radius)
{
    if (!v || (kind != 0 && kind != 1) || nx == 0 || ny == 0 || !in || !radius)
        return -1;
    if (kind)
        feature_plain_direct_grid<double>(*v, nx, ny, (fs_feature_in_f64 *)in, (double *)radius);
    else
        feature_plain_direct_grid<float>(*v, nx, ny, (fs_feature_in_f32 *)in, (float *)radius);
    return 0;
}

extern "C" void fsh_feature_destroy(fsh_feature *f) { delete f; }
extern "C" int fsh_feature_is64(const fsh_feature *f) { return f->is64; }
extern "C" int fsh_feature_kind(const fsh_feature *f) { return f->kind; }
extern "C" uint64_t fsh_feature_candidates(const fsh_feature *f) { return f->is64 ? f->c64.size() : f->c32.size(); }

extern "C" uint64_t fsh_feature_next_batch(fsh_feature *f, void *in, uint64_t cap, int *mode, void *radius, uint64_t *max_iters)
{
    mpf_set_default_prec(f->prec_bits);
    *max_iters = f->max_iters;
    if (f->kind == 2) {
        *(float *)radius = feature_eval_radius_plain<float>(*f);
        return feature_next_plain<float>(*f, (fs_feature_in_f32 *)in, cap, mode);
    }
    if (f->kind == 3) {
        *(double *)radius = feature_eval_radius_plain<double>(*f);
        return feature_next_plain<double>(*f, (fs_feature_in_f64 *)in, cap, mode);
    }
    if (f->is64) {
        const hreal<double> R = feature_eval_radius<double>(*f);
        *(fs_real_hdr64 *)radius = fs_real_hdr64{R.m, R.e, 0};
        return feature_next<double>(*f, (fs_feature_in_hdr64 *)in, cap, mode);
    }
    const hreal<float> R = feature_eval_radius<float>(*f);
    *(fs_real_hdr32 *)radius = fs_real_hdr32{R.m, R.e};
    return feature_next<float>(*f, (fs_feature_in_hdr32 *)in, cap, mode);
}

extern "C" void fsh_feature_consume(fsh_feature *f, const void *out, uint64_t n)
{
    mpf_set_default_prec(f->prec_bits);
    if (f->kind == 2)
        feature_consume_plain<float>(*f, (const fs_feature_out_f32 *)out, n);
    else if (f->kind == 3)
        feature_consume_plain<double>(*f, (const fs_feature_out_f64 *)out, n);
    else if (f->is64)
        feature_consume<double>(*f, (const fs_feature_out_hdr64 *)out, n);
    else
        feature_consume<float>(*f, (const fs_feature_out_hdr32 *)out, n);
    f->batch.clear();
}

extern "C" uint64_t fsh_feature_found(const fsh_feature *f)
{
    uint64_t n = 0;
    if (f->is64) {
        for (const auto &c : f->c64)
            n += c.stage == kFound;
    } else {
        for (const auto &c : f->c32)
            n += c.stage == kFound;
    }
    return n;
}

extern "C" int fsh_feature_result(fsh_feature *f, uint64_t k, char *cx, char *cy, char *radius, size_t buflen, uint64_t *period,
                                  fs_real_hdr64 *residual2, uint32_t *grid_index)
{
    auto fill = [&](const auto *c) {
        if (!c)
            return -1;
        gmp_snprintf(cx, buflen, "%.Fe", c->cx.v);
        gmp_snprintf(cy, buflen, "%.Fe", c->cy.v);
        gmp_snprintf(radius, buflen, "%.Fe", c->radius.v);
        *period = c->period;
        *residual2 = fs_real_hdr64{c->residual2.m, c->residual2.e, 0};
        *grid_index = c->grid;
        return 0;
    };
    return f->is64 ? fill(found_at<double>(*f, k)) : fill(found_at<float>(*f, k));
}
