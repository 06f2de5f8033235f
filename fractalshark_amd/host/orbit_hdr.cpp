// orbit_hdr.cpp -- the HDRFloat<float> / HDRFloat<double> reference orbit, its accessors and test hooks, and the
// perturbation coordinates that go with it.
#include "inputs_state.hpp"

namespace {

// AddPerturbationReferencePointST<..., Periodicity, ...>, RefOrbitCalc.cpp:423-647, for T = HDRFloat<F>,
// PerturbExtras::Disable, ReuseMode::DontSaveForReuse.
// compression_exp < 0: PerturbExtras::Disable.  Otherwise PerturbExtras::SimpleCompression with
// CompressionError = T(10^compression_exp) (RefOrbitCompressor, PerturbationResults.cpp:2334-2381; default exponent 20,
// Fractal.h:138-141).
template <class F>
void build_orbit(const fsh_view &vw, uint64_t max_iter, bool periodicity, OrbitT<F> &ob, int compression_exp = -1)
{
    mpf_set_default_prec(vw.prec_bits);
    ob.prec_bits = vw.prec_bits;
    // RefOrbitCalc.cpp:244-249: guess = bbox midpoint
    {
        Mp two = Mp::from_ui(2);
        ob.cx = (vw.maxX + vw.minX) / two;
        ob.cy = (vw.maxY + vw.minY) / two;
    }
    // PerturbationResults::InitResults, PerturbationResults.cpp:812-884
    {
        Mp delta = vw.maxY - vw.minY;
        const hreal<F> radiusY = hr_div(hr_from_mpf<F>(delta.v), hr_from_mant<F>(F(2)));
        ob.maxRadius = hr_reduced(radiusY);
        ob.orbitXLow = hr_from_mpf<F>(ob.cx.v);
        ob.orbitYLow = hr_from_mpf<F>(ob.cy.v);
    }
    ob.x.clear();
    ob.y.clear();
    ob.x.push_back(hr_zero<F>());
    ob.y.push_back(hr_zero<F>());
    ob.bad.assign(1, 0);
    const hreal<F> small_float = hr_from_mant<F>((F)1.1754944e-38); // T((SubType)1.1754944e-38), :472
    const F glitch = (F)0.0000001;                                  // :474
    ob.period = 0;
    ob.compressed = compression_exp >= 0;
    ob.wp_index.assign(1, 0);
    ob.wp_x.assign(1, hr_zero<F>());
    ob.wp_y.assign(1, hr_zero<F>());
    uint64_t count = 1; // m_UncompressedItersInOrbit
    hreal<F> rc_zx = ob.orbitXLow, rc_zy = ob.orbitYLow;
    const hreal<F> rc_err = hr_from_number<F>((F)std::pow(10.0, compression_exp));

    MpStepper s(ob.cx, ob.cy);

    hreal<F> dzdcX = hr_from_number<F>(F(1));
    hreal<F> dzdcY = hr_from_number<F>(F(0));
    hreal<F> cx_cast, cy_cast;
    {
        long e;
        double m = mpf_get_d_2exp(&e, s.cx);
        cx_cast = hr_raw<F>((int32_t)e, (F)m);
        m = mpf_get_d_2exp(&e, s.cy);
        cy_cast = hr_raw<F>((int32_t)e, (F)m);
    }
    const hreal<F> HighOne = hr_from_number<F>(F(1));
    const hreal<F> HighTwo = hr_from_number<F>(F(2));
    const hreal<F> TwoFiftySix = hr_from_number<F>(F(256));

    for (uint64_t i = 0; i < max_iter; i++) {
        hreal<F> double_zx = hr_from_mpf<F>(s.zx);
        hreal<F> double_zy = hr_from_mpf<F>(s.zy);
        if (!ob.compressed) {
            ob.x.push_back(double_zx);
            ob.y.push_back(double_zy);
        } else {
            // MaybeAddCompressedIteration({double_zx, double_zy, i + 1})
            const hreal<F> errX = hr_sub(rc_zx, double_zx);
            const hreal<F> errY = hr_sub(rc_zy, double_zy);
            const hreal<F> norm_z = hr_reduced(hr_add(hr_mul(double_zx, double_zx), hr_mul(double_zy, double_zy)));
            const hreal<F> err = hr_reduced(hr_mul(hr_add(hr_mul(errX, errX), hr_mul(errY, errY)), rc_err));
            if (hr_cmp_pos(err, norm_z) >= 0) {
                ob.wp_index.push_back(i + 1);
                ob.wp_x.push_back(double_zx);
                ob.wp_y.push_back(double_zy);
                rc_zx = double_zx;
                rc_zy = double_zy;
            }
            rc_one_iter(rc_zx, rc_zy, ob.orbitXLow, ob.orbitYLow);
        }
        count++;
        {
            // PerturbExtras::Bad, RefOrbitCalc.cpp:550-562: entries whose parts or norm underflow a binary32
            const hreal<F> sq_x = hr_mul(double_zx, double_zx);
            const hreal<F> sq_y = hr_mul(double_zy, double_zy);
            const hreal<F> norm = hr_reduced(hr_mul(hr_add(sq_x, sq_y), hr_from_mant<F>(glitch)));
            // (T)mpf_get_d(z): templated HDRFloat(const U) with U = double -- the zero test is on the double, the
            // normalisation on its cast to SubType (HDRFloat.h:295-326)
            auto from_double = [](double d) {
                if (d == 0.0)
                    return hr_zero<F>();
                const F v = (F)d;
                const auto bits = to_bits<F>(v);
                const int32_t fe = (int32_t)((bits & fbits<F>::kExpMask) >> fbits<F>::kShift) - fbits<F>::kBias;
                return hreal<F>{from_bits<F>((bits & fbits<F>::kKeepMask) | fbits<F>::kOneExp), fe};
            };
            const hreal<F> zx_reduced = hr_reduced(hr_abs(from_double(mpf_get_d(s.zx))));
            const hreal<F> zy_reduced = hr_reduced(hr_abs(from_double(mpf_get_d(s.zy))));
            const bool underflow = hr_cmp_pos(zx_reduced, small_float) <= 0 || hr_cmp_pos(zy_reduced, small_float) <= 0 ||
                                   hr_cmp_pos(norm, small_float) <= 0;
            ob.bad.push_back(underflow ? 1 : 0);
        }

        if (periodicity) {
            hr_reduce(dzdcX);
            const hreal<F> dzdcX1 = hr_abs(dzdcX);
            hr_reduce(dzdcY);
            const hreal<F> dzdcY1 = hr_abs(dzdcY);
            hr_reduce(double_zx);
            const hreal<F> zxCopy1 = hr_abs(double_zx);
            hr_reduce(double_zy);
            const hreal<F> zyCopy1 = hr_abs(double_zy);
            const hreal<F> n2 = hr_max_pos(zxCopy1, zyCopy1); // HdrMaxPositiveReduced
            const hreal<F> r0 = hr_max_pos(dzdcX1, dzdcY1);
            hreal<F> n3 = hr_mul(hr_mul(ob.maxRadius, r0), HighTwo);
            hr_reduce(n3);
            if (hr_cmp_pos(n2, n3) < 0) {
                ob.period = count; // GetCountOrbitEntries()
                break;
            } else {
                const hreal<F> dzdcXOrig = dzdcX;
                dzdcX = hr_add(hr_mul(HighTwo, hr_sub(hr_mul(double_zx, dzdcX), hr_mul(double_zy, dzdcY))), HighOne);
                dzdcY = hr_mul(HighTwo, hr_add(hr_mul(double_zx, dzdcY), hr_mul(double_zy, dzdcXOrig)));
            }
        }

        s.step();

        // RefOrbitCalc.cpp:616-622: tests z_i + c (not z_{i+1}), unreduced, against 256.
        const hreal<F> tempZX = hr_add(double_zx, cx_cast);
        const hreal<F> tempZY = hr_add(double_zy, cy_cast);
        const hreal<F> zn = hr_add(hr_mul(tempZX, tempZX), hr_mul(tempZY, tempZY));
        if (hr_cmp_pos(zn, TwoFiftySix) > 0)
            break;
    }
    ob.bad.back() = 0; // results->SetBad(false), RefOrbitCalc.cpp:625-627

    if (ob.compressed) {
        // What every consumer of a compressed orbit sees through RuntimeDecompressor::GetCompressedComplex
        // (PerturbationResultsHelpers.h:46-161): the waypoint at or below the index, advanced with runOneIter.  The
        // cache in that function only avoids recomputation; the value at an index is a pure function of the waypoints.
        ob.x.assign(count, hr_zero<F>());
        ob.y.assign(count, hr_zero<F>());
        for (size_t k = 0; k < ob.wp_index.size(); k++) {
            const uint64_t i0 = ob.wp_index[k];
            const uint64_t i1 = k + 1 < ob.wp_index.size() ? ob.wp_index[k + 1] : count;
            hreal<F> zx_ = ob.wp_x[k], zy_ = ob.wp_y[k];
            for (uint64_t i = i0; i < i1; i++) {
                ob.x[i] = zx_;
                ob.y[i] = zy_;
                rc_one_iter(zx_, zy_, ob.orbitXLow, ob.orbitYLow);
            }
        }
    }
}

} // namespace

extern "C" fsh_orbit *fsh_orbit_create_ex(const fsh_view *v, int is64, uint64_t max_iter, int periodicity,
                                          int compression_exp)
{
    auto ob = std::make_unique<fsh_orbit>();
    ob->is64 = is64;
    if (is64)
        build_orbit<double>(*v, max_iter, periodicity != 0, ob->d, compression_exp);
    else
        build_orbit<float>(*v, max_iter, periodicity != 0, ob->f, compression_exp);
    return ob.release();
}
extern "C" fsh_orbit *fsh_orbit_create(const fsh_view *v, int is64, uint64_t max_iter, int periodicity)
{
    return fsh_orbit_create_ex(v, is64, max_iter, periodicity, -1);
}
extern "C" int fsh_orbit_is64(const fsh_orbit *o) { return o->is64; }
extern "C" int fsh_orbit_is_compressed(const fsh_orbit *o) { return (o->is64 ? o->d.compressed : o->f.compressed) ? 1 : 0; }
extern "C" uint64_t fsh_orbit_compressed_count(const fsh_orbit *o)
{
    return o->is64 ? o->d.wp_index.size() : o->f.wp_index.size();
}
// GPUReferenceIter<HDRFloat<float>, SimpleCompression>[] (24 B: index, x, y) -- what FractalShark's compressed
// PerturbationResults holds and what fs_upload_orbit_compressed consumes.
extern "C" const fs_orbit_hdr32_rc *fsh_orbit_compressed_data_hdr32(fsh_orbit *o)
{
    if (o->is64 || !o->f.compressed)
        return nullptr;
    auto &ob = o->f;
    if (ob.packed_rc32.size() != ob.wp_index.size()) {
        ob.packed_rc32.resize(ob.wp_index.size());
        for (size_t k = 0; k < ob.wp_index.size(); k++)
            ob.packed_rc32[k] = fs_orbit_hdr32_rc{ob.wp_index[k], ob.wp_x[k].m, ob.wp_x[k].e, ob.wp_y[k].e, ob.wp_y[k].m};
    }
    return ob.packed_rc32.data();
}
extern "C" const fs_orbit_hdr64_rc *fsh_orbit_compressed_data_hdr64(fsh_orbit *o)
{
    if (!o->is64 || !o->d.compressed)
        return nullptr;
    auto &ob = o->d;
    if (ob.packed_rc64.size() != ob.wp_index.size()) {
        ob.packed_rc64.resize(ob.wp_index.size());
        for (size_t k = 0; k < ob.wp_index.size(); k++)
            ob.packed_rc64[k] =
                fs_orbit_hdr64_rc{ob.wp_index[k], ob.wp_x[k].m, ob.wp_x[k].e, 0, ob.wp_y[k].e, 0, ob.wp_y[k].m};
    }
    return ob.packed_rc64.data();
}
extern "C" void fsh_orbit_low_hdr64(const fsh_orbit *o, fs_real_hdr64 out[2])
{
    out[0] = fs_real_hdr64{o->d.orbitXLow.m, o->d.orbitXLow.e, 0};
    out[1] = fs_real_hdr64{o->d.orbitYLow.m, o->d.orbitYLow.e, 0};
}
extern "C" void fsh_orbit_low_hdr32(const fsh_orbit *o, fs_real_hdr32 out[2])
{
    out[0] = fs_real_hdr32{o->f.orbitXLow.m, o->f.orbitXLow.e};
    out[1] = fs_real_hdr32{o->f.orbitYLow.m, o->f.orbitYLow.e};
}
extern "C" void fsh_orbit_destroy(fsh_orbit *o) { delete o; }
extern "C" uint64_t fsh_orbit_count(const fsh_orbit *o) { return o->is64 ? o->d.x.size() : o->f.x.size(); }
// Test hook: entries idx[k] of the (uncompressed) orbit scaled by 2^exp2[k].  The result is no longer the orbit of any view;
// it is an orbit-shaped input with period boundaries where a test wants them (what the LA builders make of adjacent deep
// minima, of a minimum right behind a worker's first index...).  Returns the number of entries changed.
extern "C" uint64_t fsh_orbit_scale_entries(fsh_orbit *o, const uint64_t *idx, const int32_t *exp2, uint64_t n)
{
    uint64_t changed = 0;
    auto apply = [&](auto &ob) {
        if (ob.compressed)
            return;
        for (uint64_t k = 0; k < n; k++) {
            if (idx[k] >= ob.x.size())
                continue;
            ob.x[idx[k]].e += exp2[k];
            ob.y[idx[k]].e += exp2[k];
            changed++;
        }
        ob.packed32.clear();
        ob.packed64.clear();
    };
    if (o->is64)
        apply(o->d);
    else
        apply(o->f);
    return changed;
}
extern "C" uint64_t fsh_orbit_scale_parts(fsh_orbit *o, const uint64_t *idx, const int32_t *exp2_re, const int32_t *exp2_im, uint64_t n)
{
    uint64_t changed = 0;
    auto apply = [&](auto &ob) {
        if (ob.compressed)
            return;
        for (uint64_t k = 0; k < n; k++) {
            if (idx[k] >= ob.x.size())
                continue;
            ob.x[idx[k]].e += exp2_re[k];
            ob.y[idx[k]].e += exp2_im[k];
            changed++;
        }
        ob.packed32.clear();
        ob.packed64.clear();
    };
    if (o->is64)
        apply(o->d);
    else
        apply(o->f);
    return changed;
}
extern "C" uint64_t fsh_orbit_period(const fsh_orbit *o) { return o->is64 ? o->d.period : o->f.period; }

extern "C" const fs_orbit_hdr32 *fsh_orbit_data_hdr32(fsh_orbit *o)
{
    if (o->is64)
        return nullptr;
    auto &ob = o->f;
    if (ob.packed32.size() != ob.x.size()) {
        ob.packed32.resize(ob.x.size());
        for (size_t i = 0; i < ob.x.size(); i++)
            ob.packed32[i] = fs_orbit_hdr32{ob.x[i].m, ob.x[i].e, ob.y[i].e, ob.y[i].m};
    }
    return ob.packed32.data();
}

extern "C" const fs_orbit_hdr64 *fsh_orbit_data_hdr64(fsh_orbit *o)
{
    if (!o->is64)
        return nullptr;
    auto &ob = o->d;
    if (ob.packed64.size() != ob.x.size()) {
        ob.packed64.resize(ob.x.size());
        for (size_t i = 0; i < ob.x.size(); i++)
            ob.packed64[i] = fs_orbit_hdr64{ob.x[i].m, ob.x[i].e, 0, ob.y[i].e, 0, ob.y[i].m};
    }
    return ob.packed64.data();
}

// PerturbExtras::Bad orbits for the scaled kernel (GpuHDRx32PerturbedScaled): the HDRFloat<float> orbit with its flags,
// and its binary32 copy (RefOrbitCalc::CopyUsefulPerturbationResults -> CopyFullOrbitVector, PerturbationResults.cpp:
// 239-262: (float)x = HDRFloat::operator T() = mantissa * getMultiplier(exp), HDRFloat.h:557-568).
extern "C" const fs_orbit_hdr32_bad *fsh_orbit_data_hdr32_bad(fsh_orbit *o)
{
    if (o->is64)
        return nullptr;
    auto &ob = o->f;
    if (ob.packed32_bad.size() != ob.x.size()) {
        ob.packed32_bad.resize(ob.x.size());
        for (size_t i = 0; i < ob.x.size(); i++)
            ob.packed32_bad[i] = fs_orbit_hdr32_bad{ob.bad[i], 0u, ob.x[i].m, ob.x[i].e, ob.y[i].e, ob.y[i].m};
    }
    return ob.packed32_bad.data();
}
extern "C" const fs_orbit_f32_bad *fsh_orbit_data_f32_bad(fsh_orbit *o)
{
    if (o->is64)
        return nullptr;
    auto &ob = o->f;
    if (ob.packed_f32_bad.size() != ob.x.size()) {
        ob.packed_f32_bad.resize(ob.x.size());
        for (size_t i = 0; i < ob.x.size(); i++)
            ob.packed_f32_bad[i] = fs_orbit_f32_bad{ob.bad[i] != 0 ? 1u : 0u, 0u, hr_to_native(ob.x[i]), hr_to_native(ob.y[i])};
    }
    return ob.packed_f32_bad.data();
}
extern "C" uint64_t fsh_orbit_bad_count(const fsh_orbit *o)
{
    uint64_t n = 0;
    for (uint8_t b : (o->is64 ? o->d.bad : o->f.bad))
        n += b;
    return n;
}

extern "C" void fsh_orbit_max_radius_hdr64(const fsh_orbit *o, fs_real_hdr64 *out)
{
    out->m = o->d.maxRadius.m;
    out->e = o->d.maxRadius.e;
    out->pad_ = 0;
}
extern "C" void fsh_orbit_max_radius_hdr32(const fsh_orbit *o, fs_real_hdr32 *out)
{
    out->m = o->f.maxRadius.m;
    out->e = o->f.maxRadius.e;
}

// dx, dy, centerX, centerY for the perturbation paths -- Fractal.cpp:2230-2238 / 2513-2521:
//   dx = Reduce(T((maxX-minX)/HP(W*AA))), centerX = Reduce(T(refX - minX)), centerY = Reduce(T(refY - maxY)).
template <class F> static void perturb_coords(const fsh_view &v, const OrbitT<F> &ob, uint32_t w_aa, uint32_t h_aa,
                                              hreal<F> out[4])
{
    mpf_set_default_prec(v.prec_bits);
    Mp dx = (v.maxX - v.minX) / Mp::from_ui(w_aa);
    Mp dy = (v.maxY - v.minY) / Mp::from_ui(h_aa);
    Mp cX = ob.cx - v.minX;
    Mp cY = ob.cy - v.maxY;
    out[0] = hr_reduced(hr_from_mpf<F>(dx.v));
    out[1] = hr_reduced(hr_from_mpf<F>(dy.v));
    out[2] = hr_reduced(hr_from_mpf<F>(cX.v));
    out[3] = hr_reduced(hr_from_mpf<F>(cY.v));
}

extern "C" void fsh_view_coords_perturb_hdr32(const fsh_view *v, const fsh_orbit *o, uint32_t w_aa, uint32_t h_aa,
                                              fs_real_hdr32 out[4])
{
    hreal<float> t[4];
    perturb_coords<float>(*v, o->f, w_aa, h_aa, t);
    for (int i = 0; i < 4; i++)
        out[i] = fs_real_hdr32{t[i].m, t[i].e};
}

extern "C" void fsh_view_coords_perturb_hdr64(const fsh_view *v, const fsh_orbit *o, uint32_t w_aa, uint32_t h_aa,
                                              fs_real_hdr64 out[4])
{
    hreal<double> t[4];
    perturb_coords<double>(*v, o->d, w_aa, h_aa, t);
    for (int i = 0; i < 4; i++)
        out[i] = fs_real_hdr64{t[i].m, t[i].e, 0};
}
