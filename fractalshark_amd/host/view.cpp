// view.cpp -- the view: bounding box -> precision, squared box, centre and zoom; the coordinate forms the kernels take;
// the AutoZoomer's next view; the exact renderer's axes.
#include "inputs_state.hpp"

namespace {

// PointZoomBBConverter::SquareAspectRatio, PointZoomBBConverter.cpp:271-330.
void square_aspect(fsh_view &vw, size_t scrnWidth, size_t scrnHeight)
{
    if (scrnWidth == 0 || scrnHeight == 0)
        return;
    const uint64_t prec = vw.ptX.prec();
    Mp ratio(prec, 0), mwidth(prec, 0), height(prec, 0), tmp(prec, 0);
    {
        Mp w = Mp::from_ui(scrnWidth);
        Mp h = Mp::from_ui(scrnHeight);
        mpf_div(ratio.v, w.v, h.v);
    }
    mpf_sub(mwidth.v, vw.maxX.v, vw.minX.v);
    mpf_div(mwidth.v, mwidth.v, ratio.v);
    mpf_sub(height.v, vw.maxY.v, vw.minY.v);

    if (mpf_cmp(height.v, mwidth.v) > 0) {
        mpf_sub(tmp.v, height.v, mwidth.v);
        mpf_mul(tmp.v, ratio.v, tmp.v);
        mpf_div_ui(tmp.v, tmp.v, 2);
        mpf_sub(vw.minX.v, vw.minX.v, tmp.v);
        mpf_add(vw.maxX.v, vw.maxX.v, tmp.v);
    } else if (mpf_cmp(height.v, mwidth.v) < 0) {
        mpf_sub(tmp.v, mwidth.v, height.v);
        mpf_div_ui(tmp.v, tmp.v, 2);
        mpf_sub(vw.minY.v, vw.minY.v, tmp.v);
        mpf_add(vw.maxY.v, vw.maxY.v, tmp.v);
    }
    mpf_add(vw.ptX.v, vw.minX.v, vw.maxX.v);
    mpf_div_ui(vw.ptX.v, vw.ptX.v, 2);
    mpf_add(vw.ptY.v, vw.minY.v, vw.maxY.v);
    mpf_div_ui(vw.ptY.v, vw.ptY.v, 2);

    Mp deltaY(prec, 0);
    mpf_sub(deltaY.v, vw.maxY.v, vw.minY.v);
    if (mpf_cmp_ui(deltaY.v, 0) == 0) {
        vw.zoom = Mp::from_ui(1);
    } else {
        Mp two = Mp::from_ui(2);
        mpf_div(vw.zoom.v, two.v, deltaY.v);
        mpf_mul_ui(vw.zoom.v, vw.zoom.v, 2);
    }
}

} // namespace

extern "C" fsh_view *fsh_view_create(const char *minX, const char *minY, const char *maxX, const char *maxY,
                                     uint32_t width, uint32_t height)
{
    // GetViewPreset: coordinates are parsed at 1,000,000 bits (FractalViewPresets.cpp:11-12).
    mpf_set_default_prec(1000000);
    auto vw = std::make_unique<fsh_view>();
    vw->width = width;
    vw->height = height;
    vw->minX = Mp::from_str(minX);
    vw->minY = Mp::from_str(minY);
    vw->maxX = Mp::from_str(maxX);
    vw->maxY = Mp::from_str(maxY);
    return finish_view(std::move(vw), true);
}

fsh_view *finish_view(std::unique_ptr<fsh_view> vw, bool from_box)
{
    const uint32_t width = vw->width, height = vw->height;
    // PointZoomBBConverter(minX,minY,maxX,maxY), PointZoomBBConverter.cpp:26-53
    if (from_box) {
        Mp two = Mp::from_ui(2);
        vw->ptX = (vw->minX + vw->maxX) / two;
        vw->ptY = (vw->minY + vw->maxY) / two;
        Mp deltaY = vw->maxY - vw->minY;
        if (mpf_cmp_ui(deltaY.v, 0) == 0) {
            vw->zoom = Mp::from_ui(1);
        } else {
            Mp zf = Mp::from_ui(2) / deltaY;
            Mp zf2(zf.prec(), 0);
            mpf_mul(zf2.v, zf.v, two.v);
            vw->zoom = zf2;
        }
    }
    // Fractal::SetPrecision -> PrecisionCalculator::GetPrecision (PrecisionCalculator.cpp:21-107);
    // RequiresReuse() is false for the ST algorithms this file implements.
    {
        Mp dX = mp_abs(vw->maxX - vw->minX);
        Mp dY = mp_abs(vw->maxY - vw->minY);
        const hreal<double> tx = hr_from_mpf<double>(dX.v);
        const hreal<double> ty = hr_from_mpf<double>(dY.v);
        uint64_t larger = (uint64_t)std::max(std::abs(tx.e), std::abs(ty.e));
        larger += 120; // AuthoritativeMinExtraPrecisionInBits, HighPrecision.h
        vw->prec_bits = larger;
    }
    // PointZoomBBConverter::SetPrecision, PointZoomBBConverter.cpp:100-117
    mpf_set_default_prec(vw->prec_bits);
    vw->minX.set_prec(vw->prec_bits);
    vw->minY.set_prec(vw->prec_bits);
    vw->maxX.set_prec(vw->prec_bits);
    vw->maxY.set_prec(vw->prec_bits);
    vw->ptX.set_prec(vw->prec_bits);
    vw->ptY.set_prec(vw->prec_bits);
    vw->zoom.set_prec(vw->prec_bits);
    square_aspect(*vw, width, height);
    return vw.release();
}

// The AutoZoomer's next view (AutoZoomer.cpp:406-412) around the screen point (x, y) of the antialiased w_aa x h_aa frame:
// guess = (minX + x (maxX - minX) / w_aa, maxY - y (maxY - minY) / h_aa), box = guess +- (width, height) / divisor, in mpf at the
// view's precision; then what a new view gets (finish_view: precision for the new depth, aspect squaring).  A RESTATEMENT of
// X/YFromScreenToCalc<true> (PointZoomBBConverter.cpp:339-354): the reference goes through OriginX = w / (maxX - minX) * -minX,
// algebraically the same point; neither form can be pinned against the other to the last bit of an mpf.
extern "C" fsh_view *fsh_view_autozoom_next(const fsh_view *v, double x, double y, uint32_t w_aa, uint32_t h_aa, uint32_t divisor)
{
    if (!v || !w_aa || !h_aa || !divisor || !(x == x) || !(y == y) || std::isinf(x) || std::isinf(y))
        return nullptr;
    mpf_set_default_prec(v->prec_bits);
    const uint64_t prec = v->prec_bits;
    Mp width = v->maxX - v->minX, height = v->maxY - v->minY;
    Mp px(prec, 0), py(prec, 0), gx(prec, 0), gy(prec, 0);
    mpf_set_d(px.v, x);
    mpf_set_d(py.v, y);
    mpf_mul(gx.v, px.v, width.v);
    mpf_div_ui(gx.v, gx.v, w_aa);
    mpf_add(gx.v, v->minX.v, gx.v);
    mpf_mul(gy.v, py.v, height.v);
    mpf_div_ui(gy.v, gy.v, h_aa);
    mpf_sub(gy.v, v->maxY.v, gy.v);
    Mp half_w(prec, 0), half_h(prec, 0);
    mpf_div_ui(half_w.v, width.v, divisor);
    mpf_div_ui(half_h.v, height.v, divisor);
    auto nv = std::make_unique<fsh_view>();
    nv->width = v->width;
    nv->height = v->height;
    nv->minX = gx - half_w;
    nv->minY = gy - half_h;
    nv->maxX = gx + half_w;
    nv->maxY = gy + half_h;
    return finish_view(std::move(nv), true);
}

extern "C" void fsh_view_destroy(fsh_view *v) { delete v; }
extern "C" uint64_t fsh_view_precision_bits(const fsh_view *v) { return v->prec_bits; }

extern "C" int fsh_view_bbox_str(const fsh_view *v, int which, char *buf, size_t buflen)
{
    const Mp *p = which == 0 ? &v->minX : which == 1 ? &v->minY : which == 2 ? &v->maxX : &v->maxY;
    return gmp_snprintf(buf, buflen, "%.Fe", p->v);
}

// ------------------------------------------------------------------ exact renderer axes (this project's addition)
namespace {

// "[-]d.ddde[+-]XX" or plain "[-]ddd.ddd" -> the exact rational it denotes
bool decimal_to_mpq(const char *s, mpq_t out)
{
    std::string digits;
    bool neg = false, point = false;
    long frac = 0, exp10 = 0;
    const char *p = s;
    if (*p == '-' || *p == '+')
        neg = *p++ == '-';
    for (; *p; p++) {
        if (*p >= '0' && *p <= '9') {
            digits.push_back(*p);
            frac += point ? 1 : 0;
        } else if (*p == '.' && !point) {
            point = true;
        } else if (*p == 'e' || *p == 'E') {
            char *end = nullptr;
            exp10 = strtol(p + 1, &end, 10);
            if (end == p + 1 || *end)
                return false;
            break;
        } else {
            return false;
        }
    }
    if (digits.empty())
        return false;
    mpz_t ten;
    mpz_init(ten);
    mpz_set_str(mpq_numref(out), digits.c_str(), 10);
    mpz_set_ui(mpq_denref(out), 1);
    if (neg)
        mpz_neg(mpq_numref(out), mpq_numref(out));
    const long e = exp10 - frac;
    mpz_ui_pow_ui(ten, 10, (unsigned long)(e < 0 ? -e : e));
    if (e < 0)
        mpz_set(mpq_denref(out), ten);
    else
        mpz_mul(mpq_numref(out), mpq_numref(out), ten);
    mpz_clear(ten);
    mpq_canonicalize(out);
    return true;
}

// floor(q 2^F) as `limbs` two's-complement limbs at out[l * stride]; false when it does not fit
bool put_fixed(const mpq_t q, uint32_t F, uint32_t limbs, uint32_t *out, size_t stride, mpz_t t, mpz_t lim)
{
    mpz_mul_2exp(t, mpq_numref(q), F);
    mpz_fdiv_q(t, t, mpq_denref(q));
    mpz_set_ui(lim, 1);
    mpz_mul_2exp(lim, lim, 32 * limbs - 1);
    if (mpz_cmp(t, lim) >= 0)
        return false;
    mpz_neg(lim, lim);
    if (mpz_cmp(t, lim) < 0)
        return false;
    if (mpz_sgn(t) < 0) { // t + 2^(32 limbs)
        mpz_mul_2exp(lim, lim, 1);
        mpz_sub(t, t, lim);
    }
    for (uint32_t l = 0; l < limbs; l++) {
        out[l * stride] = (uint32_t)mpz_get_ui(t);
        mpz_fdiv_q_2exp(t, t, 32);
    }
    return true;
}

} // namespace

extern "C" int fsh_view_exact_axes(const fsh_view *v, uint32_t w_aa, uint32_t h_aa, uint32_t frac_bits, int shift_level,
                                   uint32_t limbs, uint32_t *cx3, uint32_t *cy3)
{
    if (!v || !w_aa || !h_aa || !limbs || !cx3 || !cy3)
        return -1;
    mpq_t b[4], span[2], q, c, sh;
    mpz_t t, lim;
    for (auto &x : b)
        mpq_init(x);
    mpq_inits(span[0], span[1], q, c, sh, nullptr);
    mpz_inits(t, lim, nullptr);
    bool ok = true;
    for (int k = 0; k < 4 && ok; k++) {
        char one[1];
        const int n = fsh_view_bbox_str(v, k, one, sizeof one);
        std::string s((size_t)(n > 0 ? n : 0) + 1, '\0');
        ok = n > 0 && fsh_view_bbox_str(v, k, &s[0], s.size()) == n && decimal_to_mpq(s.c_str(), b[k]);
    }
    if (ok) {
        mpq_sub(span[0], b[2], b[0]); // maxX - minX
        mpq_sub(span[1], b[3], b[1]); // maxY - minY
        mpq_set(sh, span[0]);
        if (shift_level >= 0)
            mpq_div_2exp(sh, sh, (mp_bitcnt_t)shift_level);
        const int n_axes = shift_level >= 0 ? 3 : 1;
        for (int axis = 0; axis < 2 && ok; axis++) {
            const uint32_t n = axis == 0 ? w_aa : h_aa;
            uint32_t *out = axis == 0 ? cx3 : cy3;
            for (uint32_t i = 0; i < n && ok; i++) {
                mpq_set_ui(q, i, n);
                mpq_canonicalize(q);
                mpq_mul(c, span[axis], q);
                if (axis == 0)
                    mpq_add(c, b[0], c);
                else
                    mpq_sub(c, b[3], c);
                for (int a = 0; a < n_axes && ok; a++) {
                    if (a == 0)
                        mpq_set(q, c);
                    else if (a == 1)
                        mpq_add(q, c, sh);
                    else
                        mpq_sub(q, c, sh);
                    ok = put_fixed(q, frac_bits, limbs, out + (size_t)a * limbs * n + i, n, t, lim);
                }
            }
        }
    }
    for (auto &x : b)
        mpq_clear(x);
    mpq_clears(span[0], span[1], q, c, sh, nullptr);
    mpz_clears(t, lim, nullptr);
    return ok ? 0 : -1;
}

// Cpu64 / direct kernels: dx, dy, minX, maxY as doubles -- Fractal.cpp:2118-2119,2148-2151
// (T(HighPrecision) for T=double is mpf_get_d, HighPrecision.h:497-501).
extern "C" void fsh_view_coords_direct_f64(const fsh_view *v, uint32_t w_aa, uint32_t h_aa, double out[4])
{
    mpf_set_default_prec(v->prec_bits);
    Mp dx = (v->maxX - v->minX) / Mp::from_ui(w_aa);
    Mp dy = (v->maxY - v->minY) / Mp::from_ui(h_aa);
    out[0] = mpf_get_d(dx.v);
    out[1] = mpf_get_d(dy.v);
    out[2] = mpf_get_d(v->minX.v);
    out[3] = mpf_get_d(v->maxY.v);
}

// Gpu1x32 / Gpu2x32 / Gpu2x64 (Fractal::CalcGpuFractal<IterType, float | MattDblflt | MattDbldbl>, Fractal.cpp:1896-1915):
// FillGpuCoords (:1833-1844) = {MinX, MinY, dx, dy} through FillCoord: float = (float)mpf_get_d (:1813-1818, Convert,
// HighPrecision.h:516-519); MattDblflt = head (float)src, tail (float)(src - HighPrecision{head}) (:1805-1811);
// MattDbldbl the same in double (:1774-1780).  kind: 0 = float[4], 1 = float[8], 2 = double[8], order cx, cy, dx, dy.
extern "C" void fsh_view_coords_direct_lp(const fsh_view *v, uint32_t w_aa, uint32_t h_aa, int kind, void *out)
{
    mpf_set_default_prec(v->prec_bits);
    const Mp dx = (v->maxX - v->minX) / Mp::from_ui(w_aa);
    const Mp dy = (v->maxY - v->minY) / Mp::from_ui(h_aa);
    const Mp *src[4] = {&v->minX, &v->minY, &dx, &dy};
    for (int i = 0; i < 4; i++) {
        if (kind == 0) {
            ((float *)out)[i] = (float)mpf_get_d(src[i]->v);
        } else if (kind == 1) {
            const float head = (float)mpf_get_d(src[i]->v);
            Mp h;
            mpf_set_d(h.v, (double)head);
            const Mp rest = *src[i] - h;
            ((float *)out)[2 * i] = head;
            ((float *)out)[2 * i + 1] = (float)mpf_get_d(rest.v);
        } else if (kind == 2) {
            const double head = mpf_get_d(src[i]->v);
            Mp h;
            mpf_set_d(h.v, head);
            const Mp rest = *src[i] - h;
            ((double *)out)[2 * i] = head;
            ((double *)out)[2 * i + 1] = mpf_get_d(rest.v);
        } else {
            // FillCoord(MattQFltflt / MattQDbldbl), Fractal.cpp:1751-1771: each component converts what is left after
            // subtracting the previous ones (left to right, in the precision of the source)
            Mp rest = *src[i];
            for (int k = 0; k < 4; k++) {
                const double part = kind == 3 ? (double)(float)mpf_get_d(rest.v) : mpf_get_d(rest.v);
                if (kind == 3)
                    ((float *)out)[4 * i + k] = (float)part;
                else
                    ((double *)out)[4 * i + k] = part;
                Mp h;
                mpf_set_d(h.v, part);
                rest = rest - h;
            }
        }
    }
}

// CpuHDR32 / CpuHDR64 (CalcCpuHDR<.., HDRFloat<F>, F>): dx, dy, minX, maxY as HDRFloat built from mpf
// (Fractal.cpp:2118-2119,2148-2151): mantissa in [0.5,1), NOT reduced.
template <class F> static void direct_hdr_coords(const fsh_view &v, uint32_t w_aa, uint32_t h_aa, hreal<F> out[4])
{
    mpf_set_default_prec(v.prec_bits);
    Mp dx = (v.maxX - v.minX) / Mp::from_ui(w_aa);
    Mp dy = (v.maxY - v.minY) / Mp::from_ui(h_aa);
    out[0] = hr_from_mpf<F>(dx.v);
    out[1] = hr_from_mpf<F>(dy.v);
    out[2] = hr_from_mpf<F>(v.minX.v);
    out[3] = hr_from_mpf<F>(v.maxY.v);
}
extern "C" void fsh_view_coords_direct_hdr32(const fsh_view *v, uint32_t w_aa, uint32_t h_aa, fs_real_hdr32 out[4])
{
    hreal<float> t[4];
    direct_hdr_coords<float>(*v, w_aa, h_aa, t);
    for (int i = 0; i < 4; i++)
        out[i] = fs_real_hdr32{t[i].m, t[i].e};
}
extern "C" void fsh_view_coords_direct_hdr64(const fsh_view *v, uint32_t w_aa, uint32_t h_aa, fs_real_hdr64 out[4])
{
    hreal<double> t[4];
    direct_hdr_coords<double>(*v, w_aa, h_aa, t);
    for (int i = 0; i < 4; i++)
        out[i] = fs_real_hdr64{t[i].m, t[i].e, 0};
}
