// convert_2x32.cpp -- 2x32 (HDRFloat<CudaDblflt<MattDblflt>>) and plain 2x32 (CudaDblflt) inputs, converted field-wise.
#include "inputs_state.hpp"

// The reference never computes 2x32 inputs directly: RefOrbitCalc builds the HDRFloat<double> orbit and LA table
// (ConditionalT, HDRFloat.h:1734-1760; Fractal.cpp:2771-2806) and PerturbationResults::CopyPerturbationResults /
// LAReference::CopyLAReference convert them field by field (PerturbationResults.cpp:239-347, RefOrbitCalc.cpp:2490-2513,
// LAReference.h:163-213, LAInfoDeep.h:94-107, ATInfo.h:18-30).  Each mantissa goes through MattDblflt(double)
// (dblflt.h:37-52): split into (float)d and the float remainder, then one two-sum; exponents are carried over.
namespace {

inline void df_from_double(double other, float &head, float &tail)
{
    const float a = (float)other;
    const float b = (float)(other - (double)a);
    head = a + b;
    float t1 = head - a;
    float t2 = head - t1;
    t1 = b - t1;
    t2 = a - t2;
    tail = t1 + t2;
}
inline fs_real_2x32 real_2x32(const fs_real_hdr64 &r)
{
    fs_real_2x32 o;
    df_from_double(r.m, o.head, o.tail);
    o.e = r.e;
    return o;
}
inline fs_cplx_2x32 cplx_2x32(const fs_cplx_hdr64 &c)
{
    fs_cplx_2x32 o;
    df_from_double(c.re, o.re_head, o.re_tail);
    df_from_double(c.im, o.im_head, o.im_tail);
    o.e = c.e;
    return o;
}

} // namespace

// Host-side entry points into the product's 2x32 arithmetic (csrc/df32_math.hpp is one header for host and device): the
// CPU test-suite cross-checks them bit for bit against the oracle's independent restatement.
extern "C" void fsh_df32_op(int op, const float a[2], const float b[2], float out[2])
{
    const fs::df32 x(a[0], a[1]), y(b[0], b[1]);
    const fs::df32 r = op == 0 ? x + y : (op == 1 ? x - y : x * y);
    out[0] = r.head;
    out[1] = r.tail;
}
extern "C" void fsh_hr2_reduce(fs_real_2x32 *v)
{
    fs::hreal<fs::df32> h{fs::df32(v->head, v->tail), v->e};
    fs::hr_reduce(h);
    *v = fs_real_2x32{h.m.head, h.m.tail, h.e};
}
extern "C" void fsh_hr2_add(const fs_real_2x32 *a, const fs_real_2x32 *b, int subtract, fs_real_2x32 *out)
{
    const fs::hreal<fs::df32> x{fs::df32(a->head, a->tail), a->e}, y{fs::df32(b->head, b->tail), b->e};
    const fs::hreal<fs::df32> r = subtract ? fs::hr_sub(x, y) : fs::hr_add(x, y);
    *out = fs_real_2x32{r.m.head, r.m.tail, r.e};
}
extern "C" void fsh_hc2_reduce(fs_cplx_2x32 *v)
{
    fs::hcplx<fs::df32> c{fs::df32(v->re_head, v->re_tail), fs::df32(v->im_head, v->im_tail), v->e};
    fs::hc_reduce(c);
    *v = fs_cplx_2x32{c.re.head, c.re.tail, c.im.head, c.im.tail, c.e};
}

extern "C" void fsh_convert_orbit_hdr64_to_2x32(const fs_orbit_hdr64 *in, uint64_t n, fs_orbit_2x32 *out)
{
    for (uint64_t i = 0; i < n; i++) {
        fs_orbit_2x32 o;
        df_from_double(in[i].mx, o.x_head, o.x_tail);
        o.ex = in[i].ex;
        df_from_double(in[i].my, o.y_head, o.y_tail);
        o.ey = in[i].ey;
        out[i] = o;
    }
}

extern "C" void fsh_convert_orbit_rc_hdr64_to_2x32(const fs_orbit_hdr64_rc *in, uint64_t n, fs_orbit_2x32_rc *out)
{
    for (uint64_t i = 0; i < n; i++) {
        fs_orbit_2x32_rc o;
        o.index_and_rebase = in[i].index_and_rebase & 0x7FFFFFFFFFFFFFFFull;
        df_from_double(in[i].mx, o.x_head, o.x_tail);
        o.ex = in[i].ex;
        df_from_double(in[i].my, o.y_head, o.y_tail);
        o.ey = in[i].ey;
        out[i] = o;
    }
}

// m_OrbitXLow / m_OrbitYLow of the converted results: static_cast<T>(Convert<HighPrecision, double>(m_OrbitX))
// (PerturbationResults.cpp:306-307), T = HDRFloat<CudaDblflt>: the double is split into exponent and a mantissa in
// [1, 2), the mantissa into head + tail (HDRFloat.h:341-349).
extern "C" void fsh_orbit_low_2x32(const fsh_orbit *o, fs_real_2x32 out[2])
{
    const Mp *c[2] = {o->is64 ? &o->d.cx : &o->f.cx, o->is64 ? &o->d.cy : &o->f.cy};
    for (int k = 0; k < 2; k++) {
        const double number = mpf_get_d(c[k]->v);
        fs_real_2x32 r{0.0f, 0.0f, fs::kMinBigExp};
        if (number != 0.0) {
            uint64_t bits;
            memcpy(&bits, &number, 8);
            const int64_t f_exp = (int64_t)((bits & 0x7FF0000000000000ull) >> 52) - 1023;
            const uint64_t val = (bits & 0x800FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
            double f_val;
            memcpy(&f_val, &val, 8);
            df_from_double(f_val, r.head, r.tail);
            r.e = (int32_t)f_exp;
        }
        out[k] = r;
    }
}

extern "C" void fsh_convert_la_hdr64_to_2x32(const fs_la_hdr64_u32 *in, uint64_t n, fs_la_2x32_u32 *out)
{
    for (uint64_t i = 0; i < n; i++) {
        fs_la_2x32_u32 o;
        o.Ref = cplx_2x32(in[i].Ref);
        o.ZCoeff = cplx_2x32(in[i].ZCoeff);
        o.CCoeff = cplx_2x32(in[i].CCoeff);
        o.LAThreshold = real_2x32(in[i].LAThreshold);
        o.LAThresholdC = real_2x32(in[i].LAThresholdC);
        o.MinMag = real_2x32(in[i].MinMag);
        o.StepLength = in[i].StepLength;
        o.NextStageLAIndex = in[i].NextStageLAIndex;
        out[i] = o;
    }
}

extern "C" void fsh_convert_at_hdr64_to_2x32(const fs_at_hdr64_u32 *in, fs_at_2x32_u32 *out)
{
    out->StepLength = in->StepLength;
    out->ThresholdC = real_2x32(in->ThresholdC);
    out->SqrEscapeRadius = real_2x32(in->SqrEscapeRadius);
    out->RefC = cplx_2x32(in->RefC);
    out->ZCoeff = cplx_2x32(in->ZCoeff);
    out->CCoeff = cplx_2x32(in->CCoeff);
    out->InvZCoeff = cplx_2x32(in->InvZCoeff);
    out->CCoeffSqrInvZCoeff = cplx_2x32(in->CCoeffSqrInvZCoeff);
    out->CCoeffInvZCoeff = cplx_2x32(in->CCoeffInvZCoeff);
    out->CCoeffNormSqr = real_2x32(in->CCoeffNormSqr);
    out->RefCNormSqr = real_2x32(in->RefCNormSqr);
    out->factor = real_2x32(in->factor);
}

// FillGpuCoords / FillCoord(HighPrecision, HDRFloat<CudaDblflt<MattDblflt>>&), Fractal.cpp:1826-1844,2834-2840:
// HDRFloat(const mpf_t) (HDRFloat.h:366-391) -- mantissa from mpf_get_d_2exp in [0.5,1), head = (float)m,
// tail = (float)(m - head), *not* reduced and not re-normalised.
extern "C" void fsh_view_coords_perturb_2x32(const fsh_view *v, const fsh_orbit *o, uint32_t w_aa, uint32_t h_aa,
                                             fs_real_2x32 out[4])
{
    mpf_set_default_prec(v->prec_bits);
    const Mp dx = (v->maxX - v->minX) / Mp::from_ui(w_aa);
    const Mp dy = (v->maxY - v->minY) / Mp::from_ui(h_aa);
    const Mp cX = (o->is64 ? o->d.cx : o->f.cx) - v->minX;
    const Mp cY = (o->is64 ? o->d.cy : o->f.cy) - v->maxY;
    const Mp *src[4] = {&dx, &dy, &cX, &cY};
    for (int i = 0; i < 4; i++) {
        if (mpf_cmp_ui(src[i]->v, 0) == 0) {
            out[i] = fs_real_2x32{0.0f, 0.0f, fs::kMinBigExp};
            continue;
        }
        long e;
        const double m = mpf_get_d_2exp(&e, src[i]->v);
        const float head = (float)m;
        out[i] = fs_real_2x32{head, (float)(m - (double)head), (int32_t)e};
    }
}

// field-wise double -> CudaDblflt conversions (CudaDblflt(double) = MattDblflt(double), dblflt.h:13-23)
namespace {
fs_real_p2x32 real_p2x32(double v)
{
    fs_real_p2x32 r;
    df_from_double(v, r.head, r.tail);
    return r;
}
fs_cplx_p2x32 cplx_p2x32(fs_cplx_f64 c)
{
    fs_cplx_p2x32 r;
    df_from_double(c.re, r.re_head, r.re_tail);
    df_from_double(c.im, r.im_head, r.im_tail);
    return r;
}
} // namespace

extern "C" void fsh_convert_orbit_f64_to_p2x32(const fs_orbit_f64 *in, uint64_t n, fs_orbit_p2x32 *out)
{
    for (uint64_t i = 0; i < n; i++) {
        df_from_double(in[i].x, out[i].x_head, out[i].x_tail);
        df_from_double(in[i].y, out[i].y_head, out[i].y_tail);
    }
}
// CopyFullOrbitVector's SimpleCompression arm (PerturbationResults.cpp:265-268): x, y converted, index kept
extern "C" void fsh_convert_orbit_rc_f64_to_p2x32(const fs_orbit_f64_rc *in, uint64_t n, fs_orbit_p2x32_rc *out)
{
    for (uint64_t i = 0; i < n; i++) {
        out[i].index_and_rebase = in[i].index_and_rebase & 0x7FFFFFFFFFFFFFFFull;
        df_from_double(in[i].x, out[i].x_head, out[i].x_tail);
        df_from_double(in[i].y, out[i].y_head, out[i].y_tail);
    }
}
extern "C" void fsh_convert_la_f64_to_p2x32(const fs_la_f64_u32 *in, uint64_t n, fs_la_p2x32_u32 *out)
{
    for (uint64_t i = 0; i < n; i++) {
        fs_la_p2x32_u32 o;
        o.Ref = cplx_p2x32(in[i].Ref);
        o.ZCoeff = cplx_p2x32(in[i].ZCoeff);
        o.CCoeff = cplx_p2x32(in[i].CCoeff);
        o.LAThreshold = real_p2x32(in[i].LAThreshold);
        o.LAThresholdC = real_p2x32(in[i].LAThresholdC);
        o.MinMag = real_p2x32(in[i].MinMag);
        o.StepLength = in[i].StepLength;
        o.NextStageLAIndex = in[i].NextStageLAIndex;
        out[i] = o;
    }
}
extern "C" void fsh_convert_at_f64_to_p2x32(const fs_at_f64_u32 *in, fs_at_p2x32_u32 *out)
{
    out->StepLength = in->StepLength;
    out->ThresholdC = real_p2x32(in->ThresholdC);
    out->SqrEscapeRadius = real_p2x32(in->SqrEscapeRadius);
    out->RefC = cplx_p2x32(in->RefC);
    out->ZCoeff = cplx_p2x32(in->ZCoeff);
    out->CCoeff = cplx_p2x32(in->CCoeff);
    out->InvZCoeff = cplx_p2x32(in->InvZCoeff);
    out->CCoeffSqrInvZCoeff = cplx_p2x32(in->CCoeffSqrInvZCoeff);
    out->CCoeffInvZCoeff = cplx_p2x32(in->CCoeffInvZCoeff);
    out->CCoeffNormSqr = real_p2x32(in->CCoeffNormSqr);
    out->RefCNormSqr = real_p2x32(in->RefCNormSqr);
    out->factor = real_p2x32(in->factor);
}
extern "C" void fsh_convert_coords_f64_to_p2x32(const double in[4], fs_real_p2x32 out[4])
{
    for (int i = 0; i < 4; i++)
        out[i] = real_p2x32(in[i]);
}
