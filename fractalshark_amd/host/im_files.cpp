// im_files.cpp -- Imagina ".im" files: the location form of a view, and the form that carries a reference orbit.
#include "inputs_state.hpp"

// ------------------------------------------------------------------ location form
// The reference saves / loads a view as an Imagina location file (RefOrbitCalc::SaveOrbitResults(filename),
// RefOrbitCalc.cpp:3117-3166; LoadOrbitConstInternal, :3425-3520; ImaginaOrbit.h:10-24):
//   IMFileHeader { u64 Magic = 0x000A0D56504D49FF ("\xFFIMPV\r\n\0"; "Sharks:)" = 0x536861726b733a29 for the reference's own
//                  variant), u64 Reserved = 0, u64 LocationOffset = 32, u64 ReferenceOffset = 0 (no orbit stored) }
//   at LocationOffset: HRReal halfH  = HDRFloat<double, Left, int64_t>{ double mantissa; int64 exp } = half the view's height
//                      u64 iterationLimit
//                      mpf orbitX, mpf orbitY  (the view's centre) in the MPIR raw stream form of MpirSerialization.cpp:157-187:
//                          long _mp_exp (limbs), then the limbs as one integer: int32 big-endian signed byte count +
//                          magnitude bytes, most significant first
// Files that also carry a reference orbit (ReferenceOffset != 0: the reference's MaxCompression intermediate form) are
// recognised and loaded as locations; the stored orbit is ignored (it is not needed to render: the orbit is recomputed).
namespace {

constexpr uint64_t kImMagic = 0x000A0D56504D49FFull, kSharksMagic = 0x536861726b733a29ull;
// precision a location file may ask for (bits): the view must still be expressible with int32 exponents, and GMP aborts
// (it does not throw) when asked for more than it can allocate
constexpr uint64_t kMaxImPrecisionBits = 1ull << 26;
// orbit entries a file may announce (32 bytes each while it is expanded on the host: 16 GiB)
constexpr uint64_t kMaxImOrbitEntries = 1ull << 29;

// exp_bytes = sizeof(long) of the build that wrote the file: 4 for the reference's Windows (MSVC) build and Imagina itself,
// 8 for the reference built on Linux.  Limbs are 64-bit in both (MPIR x64 / GMP), so only the field width differs.
// The integer stream under the mpf one: MpirSerialization::mpz_out_raw_stream / mpz_inp_raw_stream (MPIR's mpz_out_raw):
// a 4-byte big-endian signed header sign x byte-count, then the magnitude, most significant byte first.  Pinned by the
// reference's own byte vectors (FractalSharkTest/TestMpirSerialization.cpp:236-308, :393-428; tests/test_mpir_wire_format.py).
size_t im_write_mpz(FILE *f, mpz_srcptr Z)
{
    size_t byte_count = 0;
    const int sign = mpz_sgn(Z);
    if (sign != 0)
        byte_count = (mpz_sizeinbase(Z, 2) + 7) / 8;
    const int32_t header = sign == 0 ? 0 : (sign < 0 ? -1 : 1) * (int32_t)byte_count;
    const uint32_t u = (uint32_t)header;
    const unsigned char hdr[4] = {(unsigned char)(u >> 24), (unsigned char)(u >> 16), (unsigned char)(u >> 8), (unsigned char)u};
    fwrite(hdr, 1, 4, f);
    if (byte_count) {
        std::vector<unsigned char> buf(byte_count);
        size_t n = 0;
        mpz_export(buf.data(), &n, 1, 1, 1, 0, Z);
        fwrite(buf.data(), 1, byte_count, f);
    }
    return 4 + byte_count;
}

// Z must be initialised.  *nonzero: whether the header announced a magnitude.
bool im_read_mpz(FILE *f, mpz_ptr Z, bool *nonzero)
{
    unsigned char hdr[4];
    if (fread(hdr, 1, 4, f) != 4)
        return false;
    const int32_t raw = (int32_t)(((uint32_t)hdr[0] << 24) | ((uint32_t)hdr[1] << 16) | ((uint32_t)hdr[2] << 8) | hdr[3]);
    mpz_set_ui(Z, 0);
    if (raw != 0) {
        const size_t n = (size_t)std::abs((int64_t)raw);
        if (n > (1u << 24)) // 128 Mbit of mantissa: not a location anyone saved; the wrong exponent width reads such counts
            return false;
        std::vector<unsigned char> buf(n);
        if (fread(buf.data(), 1, n, f) != n)
            return false;
        mpz_import(Z, n, 1, 1, 1, 0, buf.data());
        if (raw < 0)
            mpz_neg(Z, Z);
    }
    if (nonzero)
        *nonzero = raw != 0;
    return true;
}

void im_write_mpf(FILE *f, mpf_srcptr X, int exp_bytes)
{
    const int64_t expt = X->_mp_exp;
    if (exp_bytes == 4) {
        const int32_t e32 = (int32_t)expt;
        fwrite(&e32, 4, 1, f);
    } else {
        fwrite(&expt, 8, 1, f);
    }
    mpz_t Z; // non-owning view of X's limbs, like the reference
    const int nz = X->_mp_size;
    Z->_mp_alloc = std::abs(nz);
    Z->_mp_size = nz;
    Z->_mp_d = X->_mp_d;
    im_write_mpz(f, Z);
}

bool im_read_mpf(FILE *f, mpf_ptr X, int exp_bytes)
{
    int64_t expt = 0;
    if (exp_bytes == 4) {
        int32_t e32;
        if (fread(&e32, 4, 1, f) != 1)
            return false;
        expt = e32;
    } else if (fread(&expt, 8, 1, f) != 1) {
        return false;
    }
    mpz_t Z;
    mpz_init(Z);
    bool nonzero = false;
    if (!im_read_mpz(f, Z, &nonzero)) {
        mpz_clear(Z);
        return false;
    }
    mpf_set_z(X, Z);
    if (nonzero)
        X->_mp_exp = (mp_exp_t)expt;
    mpz_clear(Z);
    return true;
}

struct ImHR { // Imagina::HRReal = HDRFloat<double, Left, int64_t>
    double mantissa;
    int64_t exp;
};
static_assert(sizeof(ImHR) == 16, "HRReal");

} // namespace

// The integer stream on its own, memory to memory (tests: the reference's wire-format vectors).  fsh_mpz_raw_write: the
// bytes of `value` (a number in `base`) into out[0 .. cap), returns their count (0: bad number or no room).
// fsh_mpz_raw_read: one integer from in[0 .. n), its decimal text into out_decimal; returns the bytes consumed (0: error).
extern "C" size_t fsh_mpz_raw_write(const char *value, int base, unsigned char *out, size_t cap)
{
    mpz_t z;
    if (mpz_init_set_str(z, value, base) != 0) {
        mpz_clear(z);
        return 0;
    }
    char *mem = nullptr;
    size_t len = 0;
    FILE *f = open_memstream(&mem, &len);
    size_t written = 0;
    if (f) {
        written = im_write_mpz(f, z);
        fclose(f);
        if (written != len || len > cap)
            written = 0;
        else
            memcpy(out, mem, len);
        free(mem);
    }
    mpz_clear(z);
    return written;
}
extern "C" size_t fsh_mpz_raw_read(const unsigned char *in, size_t n, char *out_decimal, size_t cap)
{
    if (n == 0)
        return 0;
    FILE *f = fmemopen(const_cast<unsigned char *>(in), n, "rb");
    if (!f)
        return 0;
    mpz_t z;
    mpz_init(z);
    size_t used = 0;
    if (im_read_mpz(f, z, nullptr) && mpz_sizeinbase(z, 10) + 2 <= cap) {
        mpz_get_str(out_decimal, 10, z);
        used = (size_t)ftell(f);
    }
    mpz_clear(z);
    fclose(f);
    return used;
}

extern "C" int fsh_view_save_im(const fsh_view *v, uint64_t iteration_limit, const char *path, int exp_bytes)
{
    if (exp_bytes != 4 && exp_bytes != 8)
        return -1;
    FILE *f = fopen(path, "wb");
    if (!f)
        return -1;
    const uint64_t header[4] = {kImMagic, 0, 32, 0};
    fwrite(header, 8, 4, f);
    // radiusY = double{maxY - minY} / 2.0; halfH = HRReal{radiusY}: the templated HDRFloat(number) constructor
    // (HDRFloat.h:295-363): zero -> {0, MIN_BIG_EXPONENT}, else mantissa in [1, 2) and the exponent beside it
    mpf_set_default_prec(v->prec_bits);
    Mp dY = v->maxY - v->minY;
    const double radiusY = mpf_get_d(dY.v) / 2.0;
    ImHR hh;
    if (radiusY == 0.0) {
        hh.mantissa = 0.0;
        hh.exp = INT16_MIN >> 3; // GenericHdrBase::MIN_BIG_EXPONENT for a TExp that is neither int32_t nor float
    } else {
        // the same bit surgery (HDRFloat.h:307-316), so that subnormal radii come out the way the reference writes them
        uint64_t bits;
        memcpy(&bits, &radiusY, 8);
        const uint64_t val = (bits & 0x800FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
        memcpy(&hh.mantissa, &val, 8);
        hh.exp = (int64_t)((bits & 0x7FF0000000000000ull) >> 52) - 1023;
    }
    fwrite(&hh, sizeof(hh), 1, f);
    fwrite(&iteration_limit, 8, 1, f);
    im_write_mpf(f, v->ptX.v, exp_bytes);
    im_write_mpf(f, v->ptY.v, exp_bytes);
    const bool ok = !ferror(f);
    fclose(f);
    return ok ? 0 : -1;
}

extern "C" fsh_view *fsh_view_load_im(const char *path, uint32_t width, uint32_t height, uint64_t *iteration_limit,
                                     int *has_orbit, int *exp_bytes_out)
{
    FILE *f = fopen(path, "rb");
    if (!f)
        return nullptr;
    uint64_t header[4];
    ImHR hh;
    uint64_t limit = 0;
    fsh_view *out = nullptr;
    if (fread(header, 8, 4, f) == 4 && (header[0] == kImMagic || header[0] == kSharksMagic) &&
        fseek(f, (long)header[2], SEEK_SET) == 0 && fread(&hh, sizeof(hh), 1, f) == 1 && fread(&limit, 8, 1, f) == 1) {
        // precision = -min(0, halfH.exp) + AuthoritativeMinExtraPrecisionInBits (RefOrbitCalc.cpp:3458-3460)
        if (hh.exp < -(int64_t)kMaxImPrecisionBits) {
            fclose(f);
            return nullptr;
        }
        const uint64_t precision = (uint64_t)(-std::min<int64_t>(0, hh.exp)) + 120u;
        mpf_set_default_prec(precision);
        Mp X(precision, 0), Y(precision, 0), H(precision, 0);
        // which `long` wrote the file: the two values must end exactly where the location section ends (the reference
        // orbit's offset, or the end of the file)
        const long at = ftell(f);
        fseek(f, 0, SEEK_END);
        const long section_end = header[3] > header[2] ? (long)header[3] : ftell(f);
        int width_ok = 0;
        for (int exp_bytes : {4, 8}) {
            fseek(f, at, SEEK_SET);
            if (im_read_mpf(f, X.v, exp_bytes) && im_read_mpf(f, Y.v, exp_bytes) && ftell(f) == section_end) {
                width_ok = exp_bytes;
                break;
            }
        }
        // halfH == 0 is what the writer stores for a view too deep for a double radius; there is no box to load
        // (the reference divides by it)
        if (width_ok && hh.mantissa != 0.0) {
            // halfH.GetHighPrecision (HDRFloat.h:396-412); the box is pt -+ Factor / zoomFactor = pt -+ halfH
            mpf_set_d(H.v, hh.mantissa);
            if (hh.exp >= 0)
                mpf_mul_2exp(H.v, H.v, (mp_bitcnt_t)hh.exp);
            else
                mpf_div_2exp(H.v, H.v, (mp_bitcnt_t)(-hh.exp));
            // zoomFactor = 2 / halfH (:3462-3465), then PointZoomBBConverter(ptX, ptY, zoomFactor): the box is
            // pt -+ Factor / zoomFactor (PointZoomBBConverter.cpp:9-24), every operation rounded at `precision`
            const Mp two = Mp::from_ui(2);
            const Mp zoom = two / H;
            const Mp r = two / zoom;
            auto vw = std::make_unique<fsh_view>();
            vw->width = width;
            vw->height = height;
            vw->ptX = X;
            vw->ptY = Y;
            vw->zoom = zoom;
            vw->minX = X - r;
            vw->minY = Y - r;
            vw->maxX = X + r;
            vw->maxY = Y + r;
            out = finish_view(std::move(vw), false);
            if (iteration_limit)
                *iteration_limit = limit;
            if (has_orbit)
                *has_orbit = header[3] != 0;
            if (exp_bytes_out)
                *exp_bytes_out = width_ok;
        }
    }
    fclose(f);
    return out;
}

// ------------------------------------------------------------------ files that carry a reference orbit
// RefOrbitCalc::SaveOrbitResults(results, filename) (RefOrbitCalc.cpp:3039-3115) writes, after the location section
// (header, halfH = the orbit's MaxRadius, iteration limit = MaxIterations - 1, centre), at ReferenceOffset:
//   ReferenceHeader { bool ExtendedRange }                                                     1 B
//   ReferenceTrivialContent { HRReal AbsolutePrecision {2, -precisionInBits}, RelativePrecision {}, ValidRadius = MaxRadius }   48 B
//   LAReferenceTrivialContent { complex<double> Refc; size_t RefIt = count - 1, MaxIt = MaxIterations - 2; bool x4
//                               (IsPeriodic = period != 0); ImaginaATInfo AT {}; size_t LAStageCount = 0 }                     192 B
//   size_t n; n x { HRReal x, HRReal y, CompressionIndexField (63-bit orbit index, 1 rebase bit) }                            40 B each
//   size_t r; r x uint64 rebase indices
// (PerturbationResults::SaveOrbitBin, PerturbationResults.cpp:2013-2082; sizes and offsets checked against the reference's
// headers in tests/test_im_orbit.py).  The waypoints are the orbit under "max compression" (PerturbationResults::
// CompressMax, :1347-1640 -- the waypoint scheme of Imagina: the orbit is re-derived by perturbing it against its own
// beginning, and a waypoint is stored where that drifts by more than sqrt(10^-CompressionErrorExp) relative, Chebyshev norm);
// the reader rebuilds the full orbit from them (LoadOrbitBin :2104-2211, DecompressMax :1660-1840, with the backwards
// Newton correction of every stretch between two waypoints).  Restated here for T = HDRFloat<float> ("Sharks:)" magic) and
// HDRFloat<double> (Imagina's magic), ExtendedRange = true.
namespace {

template <class F> struct MaxWaypoints {
    std::vector<real_t<F>> x, y;
    std::vector<uint64_t> index;
    std::vector<uint8_t> rebase;
    std::vector<uint64_t> rebases;
};

template <class R> R mc_norm(R x, R y)
{
    // HdrMaxReduced(HdrAbs(x), HdrAbs(y)) (HDRFloat.h:1477-1500: `one.compareTo(two) > 0 ? one : two`), HdrReduce
    const R ax = hr_abs(x), ay = hr_abs(y);
    return hr_reduced(hr_cmp(ax, ay) > 0 ? ax : ay);
}
template <class R> R mc_norm_times(R x, R y, R t)
{
    const R ax = hr_abs(x), ay = hr_abs(y);
    return hr_reduced(hr_mul(hr_cmp(ax, ay) > 0 ? ax : ay, t));
}
// dz' = (2 Z + dz) dz in the reference's operand order (PerturbationResults.cpp:1489-1493, 1610-1614, 1842-1848)
template <class F> void mc_dz_step(real_t<F> &dzX, real_t<F> &dzY, real_t<F> Zx, real_t<F> Zy)
{
    const real_t<F> Two = mk<F>::number(2.0);
    const real_t<F> old = dzX;
    dzX = hr_sub(hr_add(hr_sub(hr_mul(hr_mul(Two, Zx), dzX), hr_mul(hr_mul(Two, Zy), dzY)), hr_mul(dzX, dzX)), hr_mul(dzY, dzY));
    hr_reduce(dzX);
    dzY = hr_add(hr_add(hr_mul(hr_mul(Two, Zx), dzY), hr_mul(hr_mul(Two, Zy), old)), hr_mul(hr_mul(Two, old), dzY));
    hr_reduce(dzY);
}

// PerturbationResults::CompressMax, PerturbationResults.cpp:1347-1640 (includeDummy = false)
template <class F, class Orb>
MaxWaypoints<F> compress_max(const Orb &ob, real_t<F> orbitXLow, real_t<F> orbitYLow, int compression_exp)
{
    using hr = real_t<F>;
    using S = scalar_t<F>;
    MaxWaypoints<F> w;
    const uint64_t count = ob.x.size();
    const hr threshold2 = mk<F>::number((S)std::sqrt(std::pow(10.0, compression_exp)));
    const hr constant1 = hr_reduced(mk<F>::number((S)0x1.0p-4));
    const hr constant2 = hr_reduced(mk<F>::number((S)0x1.000001p0));
    hr zx = orbitXLow, zy = orbitYLow;
    auto push = [&](hr x, hr y, uint64_t i, bool rebase) {
        w.x.push_back(x), w.y.push_back(y), w.index.push_back(i), w.rebase.push_back(rebase ? 1 : 0);
    };
    uint64_t i = 1;
    for (; i < count; i++) {
        const hr outX = ob.x[i], outY = ob.y[i];
        const hr norm_z = mc_norm(outX, outY);
        if (hr_cmp_pos(norm_z, constant1) < 0) {
            zx = outX, zy = outY;
            push(outX, outY, i, true);
            break;
        } else {
            const hr err = mc_norm_times(hr_sub(zx, outX), hr_sub(zy, outY), threshold2);
            if (hr_cmp_pos(err, norm_z) >= 0) {
                zx = outX, zy = outY;
                push(outX, outY, i, false);
            }
        }
        rc_one_iter(zx, zy, orbitXLow, orbitYLow);
    }
    hr dzX = zx, dzY = zy;
    uint64_t prev_waypoint = i;
    mc_dz_step<F>(dzX, dzY, ob.x[0], ob.y[0]);
    i++;
    uint64_t j = 1;
    for (; i < count; i++, j++) {
        const hr outXi = ob.x[i], outYi = ob.y[i];
        hr outXj = ob.x[j], outYj = ob.y[j];
        zx = hr_add(dzX, outXj);
        zy = hr_add(dzY, outYj);
        const hr norm_z_orig = mc_norm(zx, zy);
        const hr norm_dz_orig = mc_norm_times(dzX, dzY, constant2);
        const hr err = mc_norm_times(hr_sub(zx, outXi), hr_sub(zy, outYi), threshold2);
        const bool condition1 = j >= prev_waypoint;
        const bool condition2 = hr_cmp_pos(err, norm_z_orig) >= 0;
        if (condition1 || condition2) {
            prev_waypoint = i;
            zx = outXi, zy = outYi;
            dzX = hr_sub(zx, outXj);
            dzY = hr_sub(zy, outYj);
            const hr norm_z = mc_norm(zx, zy), norm_dz = mc_norm(dzX, dzY);
            if (hr_cmp_pos(norm_z, norm_dz) < 0 || (i - j) * 4 < i) {
                dzX = zx, dzY = zy;
                j = 0;
                push(dzX, dzY, i, true);
            } else {
                push(dzX, dzY, i, false);
            }
        } else if (hr_cmp_pos(norm_z_orig, norm_dz_orig) < 0) {
            dzX = zx, dzY = zy;
            j = 0;
            if (!w.rebases.empty() && !w.index.empty() && w.rebases.back() > w.index.back())
                w.rebases.back() = i;
            else
                w.rebases.push_back(i);
        }
        outXj = ob.x[j], outYj = ob.y[j]; // j may have changed
        mc_dz_step<F>(dzX, dzY, outXj, outYj);
    }
    return w;
}

// PerturbationResults::DecompressMax<Disable>, PerturbationResults.cpp:1660-1850.  The waypoint and rebase lists carry the
// reader's terminators (index ~0) at their ends (LoadOrbitBin :2208-2210).
template <class F>
void decompress_max(const MaxWaypoints<F> &w, real_t<F> cxLow, real_t<F> cyLow, uint64_t target, std::vector<real_t<F>> &ox,
                    std::vector<real_t<F>> &oy)
{
    using hr = real_t<F>;
    ox.clear(), oy.clear();
    ox.reserve(target), oy.reserve(target);
    const hr Two = mk<F>::number(2.0);
    // CorrectOrbit, :1712-1760: the stretch [begin, end) is pulled onto the waypoint by a backwards Newton step per entry
    auto correct = [&](uint64_t begin, uint64_t end, hr diffX, hr diffY) {
        hr dzdcX = mk<F>::number(1.0), dzdcY = mk<F>::number(0.0);
        hr_reduce(diffX);
        hr_reduce(diffY);
        for (uint64_t i = end; i > begin;) {
            i--;
            const hr old = dzdcX;
            // dzdcX * Z.x * 2 - dzdcY * Z.y * 2 ; `* 2` is HDRFloat * int -> HDRFloat(int 2) = {1.0, 1}
            dzdcX = hr_sub(hr_mul(hr_mul(dzdcX, ox[i]), Two), hr_mul(hr_mul(dzdcY, oy[i]), Two));
            hr_reduce(dzdcX);
            dzdcY = hr_add(hr_mul(hr_mul(old, oy[i]), Two), hr_mul(hr_mul(dzdcY, ox[i]), Two));
            hr_reduce(dzdcY);
            const hr den = hr_add(hr_mul(dzdcX, dzdcX), hr_mul(dzdcY, dzdcY));
            hr resultReal = hr_div(hr_add(hr_mul(diffX, dzdcX), hr_mul(diffY, dzdcY)), den);
            hr_reduce(resultReal);
            hr resultImag = hr_div(hr_sub(hr_mul(diffY, dzdcX), hr_mul(diffX, dzdcY)), den);
            hr_reduce(resultImag);
            ox[i] = hr_reduced(hr_add(ox[i], resultReal));
            oy[i] = hr_reduced(hr_add(oy[i], resultImag));
        }
    };
    hr zx = mk<F>::zero(), zy = mk<F>::zero(); // T zx{}, zy{}
    uint64_t wp = 0, rb = 0;
    uint64_t next_index = w.index[0];
    uint64_t next_rebase = w.rebases[0];
    uint64_t i = 0, uncorrected_begin = 1;
    for (; i < target; i++) {
        if (i == next_index) {
            correct(uncorrected_begin, i, hr_sub(w.x[wp], zx), hr_sub(w.y[wp], zy));
            uncorrected_begin = i + 1;
            zx = w.x[wp], zy = w.y[wp];
            const bool rebase = w.rebase[wp] != 0;
            wp++;
            next_index = w.index[wp];
            if (rebase)
                break;
        }
        ox.push_back(zx), oy.push_back(zy);
        rc_one_iter(zx, zy, cxLow, cyLow);
    }
    uint64_t j = 0;
    hr dzX = zx, dzY = zy;
    for (; i < target; i++, j++) {
        zx = hr_add(dzX, ox[j]);
        zy = hr_add(dzY, oy[j]);
        if (i == next_index) {
            if (w.rebase[wp]) {
                dzX = zx, dzY = zy;
                j = 0;
            }
            correct(uncorrected_begin, i, hr_sub(w.x[wp], dzX), hr_sub(w.y[wp], dzY));
            uncorrected_begin = i + 1;
            dzX = w.x[wp], dzY = w.y[wp];
            zx = hr_add(dzX, ox[j]);
            zy = hr_add(dzY, oy[j]);
            wp++;
            next_index = w.index[wp];
        } else if (i == next_rebase) {
            rb++;
            next_rebase = w.rebases[rb];
            dzX = zx, dzY = zy;
            j = 0;
        } else {
            const hr norm_z = mc_norm(zx, zy), norm_dz = mc_norm(dzX, dzY);
            if (hr_cmp_pos(norm_z, norm_dz) < 0) {
                dzX = zx, dzY = zy;
                j = 0;
            }
        }
        ox.push_back(zx), oy.push_back(zy);
        mc_dz_step<F>(dzX, dzY, ox[j], oy[j]);
    }
}

template <class F> ImHR im_hr(hreal<F> v) { return ImHR{(double)v.m, (int64_t)v.e}; }
// Imagina::HRReal{T} for a plain T: the templated HDRFloat(const U number) constructor, which normalises (HDRFloat.h:295-363)
template <class T> ImHR im_hr(preal<T> v)
{
    const hreal<double> h = hr_from_number<double>((double)v.m);
    return ImHR{h.m, (int64_t)h.e};
}

// F: the number family (float / double: HDRFloat<F>, ExtendedRange = true, 40-byte waypoints of two HRReal and the index field;
// plain<float> / plain<double>: ExtendedRange = false, 24-byte waypoints of two doubles and the index field,
// PerturbationResults.cpp:2047-2075).  The magic follows the SubType (RefOrbitCalc.cpp:3052-3062).
template <class F, class Orb>
int save_im_orbit(const Orb &ob, real_t<F> orbitXLow, real_t<F> orbitYLow, uint64_t num_iterations, int compression_exp,
                  const char *path, int exp_bytes)
{
    if ((exp_bytes != 4 && exp_bytes != 8) || ob.x.size() < 2)
        return -1;
    FILE *f = fopen(path, "wb");
    if (!f)
        return -1;
    uint64_t header[4] = {sizeof(scalar_t<F>) == 4 ? kSharksMagic : kImMagic, 0, 32, 0};
    fwrite(header, 8, 4, f);
    const ImHR halfH = im_hr(ob.maxRadius); // Imagina::HRReal{results.GetMaxRadius()}
    fwrite(&halfH, sizeof(halfH), 1, f);
    const uint64_t iteration_limit = num_iterations; // GetMaxIterations() - 1, MaxIterations = NumIterations + 1 (:859)
    fwrite(&iteration_limit, 8, 1, f);
    im_write_mpf(f, ob.cx.v, exp_bytes);
    im_write_mpf(f, ob.cy.v, exp_bytes);
    const uint64_t reference_offset = (uint64_t)ftell(f);
    const MaxWaypoints<F> w = compress_max<F>(ob, orbitXLow, orbitYLow, compression_exp);
    const uint8_t extended_range = num<F>::is_plain ? 0 : 1; // results.IsHDR
    fwrite(&extended_range, 1, 1, f);
    // ReferenceTrivialContent
    const ImHR trivial[3] = {ImHR{2.0, -(int64_t)mpf_get_prec(ob.cx.v)}, ImHR{0.0, 0}, im_hr(ob.maxRadius)};
    fwrite(trivial, sizeof(ImHR), 3, f);
    // LAReferenceTrivialContent, 192 bytes: Refc @0, RefIt @16, MaxIt @24, bools @32..35 (IsPeriodic @34), AT @40, LAStageCount @184
    unsigned char la[192];
    memset(la, 0, sizeof(la));
    const double refc[2] = {mpf_get_d(ob.cx.v), mpf_get_d(ob.cy.v)};
    memcpy(la + 0, refc, 16);
    const uint64_t ref_it = ob.x.size() - 1, max_it = num_iterations + 1 - 2;
    memcpy(la + 16, &ref_it, 8);
    memcpy(la + 24, &max_it, 8);
    la[34] = ob.period != 0 ? 1 : 0;
    fwrite(la, 1, sizeof(la), f);
    const uint64_t n = w.x.size();
    fwrite(&n, 8, 1, f);
    for (uint64_t k = 0; k < n; k++) {
        if constexpr (num<F>::is_plain) {
            const double xy[2] = {(double)w.x[k].m, (double)w.y[k].m};
            fwrite(xy, sizeof(double), 2, f);
        } else {
            const ImHR xy[2] = {im_hr(w.x[k]), im_hr(w.y[k])};
            fwrite(xy, sizeof(ImHR), 2, f);
        }
        const uint64_t field = (w.index[k] & 0x7FFFFFFFFFFFFFFFull) | ((uint64_t)w.rebase[k] << 63);
        fwrite(&field, 8, 1, f);
    }
    const uint64_t r = w.rebases.size();
    fwrite(&r, 8, 1, f);
    if (r)
        fwrite(w.rebases.data(), 8, r, f);
    header[3] = reference_offset;
    fseek(f, 0, SEEK_SET);
    fwrite(header, 8, 4, f);
    const bool ok = !ferror(f);
    fclose(f);
    return ok ? 0 : -1;
}

// the stored orbit of an open file (positioned anywhere), into ob: LoadOrbitBin + DecompressMax<Disable>
template <class F, class Orb>
bool load_im_orbit(FILE *f, uint64_t reference_offset, Orb &ob, uint64_t file_iteration_limit, ImHR halfH)
{
    if (fseek(f, (long)reference_offset, SEEK_SET) != 0)
        return false;
    uint8_t extended_range = 0;
    ImHR trivial[3];
    unsigned char la[192];
    uint64_t n = 0;
    if (fread(&extended_range, 1, 1, f) != 1 || fread(trivial, sizeof(ImHR), 3, f) != 3 || fread(la, 1, sizeof(la), f) != sizeof(la) ||
        fread(&n, 8, 1, f) != 1 || (extended_range != 0) == num<F>::is_plain || n == 0 || n > (1ull << 32))
        return false;
    uint64_t ref_it;
    memcpy(&ref_it, la + 16, 8);
    // a file is untrusted input: the orbit it announces must fit the device-side 32-bit indices and may not be longer than
    // the iteration limit it was computed for (a crafted RefIt would otherwise size the vectors below)
    if (ref_it >= (1ull << 32) || (file_iteration_limit != 0 && ref_it > file_iteration_limit))
        return false;
    // ... nor longer than this host can expand (the iteration limit comes from the same file): DecompressMax sizes its vectors
    // for ref_it entries of 2 x 16 bytes, and with overcommit a crafted length ends in an OOM kill rather than a bad_alloc
    if (ref_it > kMaxImOrbitEntries)
        return false;
    const bool periodic = la[34] != 0;
    MaxWaypoints<F> w;
    auto exp_fits = [](const ImHR &h) { return h.exp >= INT32_MIN && h.exp <= INT32_MAX; };
    if (!exp_fits(halfH))
        return false;
    uint64_t prev_index = 0;
    for (uint64_t k = 0; k < n; k++) {
        ImHR xy[2];
        double pxy[2] = {0.0, 0.0};
        uint64_t field;
        if constexpr (num<F>::is_plain) {
            if (fread(pxy, sizeof(double), 2, f) != 2 || fread(&field, 8, 1, f) != 1)
                return false;
            xy[0] = xy[1] = ImHR{0.0, 0};
        } else {
            if (fread(xy, sizeof(ImHR), 2, f) != 2 || fread(&field, 8, 1, f) != 1)
                return false;
        }
        // waypoints are strictly increasing orbit positions >= 1 (entry 0 is the implicit zero start; DecompressMax reads the
        // entry BEFORE a rebasing waypoint), inside the announced orbit, with exponents that fit HDRFloat's int32
        const uint64_t idx = field & 0x7FFFFFFFFFFFFFFFull;
        if (idx == 0 || idx <= prev_index || idx > ref_it || !exp_fits(xy[0]) || !exp_fits(xy[1]))
            return false;
        prev_index = idx;
        if constexpr (num<F>::is_plain) {
            w.x.push_back(real_t<F>{(scalar_t<F>)pxy[0]}); // static_cast<T>(x), PerturbationResults.cpp:2177-2183
            w.y.push_back(real_t<F>{(scalar_t<F>)pxy[1]});
        } else {
            w.x.push_back(hreal<F>{(F)xy[0].mantissa, (int32_t)xy[0].exp});
            w.y.push_back(hreal<F>{(F)xy[1].mantissa, (int32_t)xy[1].exp});
        }
        w.index.push_back(field & 0x7FFFFFFFFFFFFFFFull);
        w.rebase.push_back((uint8_t)(field >> 63));
    }
    uint64_t r = 0;
    // every rebase is an orbit position, so a file that announces more of them than the (already bounded) orbit has entries
    // is not one CompressMax wrote -- refused BEFORE anything is allocated for it; the list itself is read in chunks, so the
    // memory that gets touched follows the bytes that are really there
    if (fread(&r, 8, 1, f) != 1 || r > ref_it + 1)
        return false;
    for (uint64_t done = 0; done < r;) {
        const uint64_t chunk = std::min<uint64_t>(r - done, 1u << 16);
        w.rebases.resize(done + chunk);
        if (fread(w.rebases.data() + done, 8, chunk, f) != chunk)
            return false;
        done += chunk;
    }
    // the reader's terminators (:2208-2210): {{}, {}, ~0ull, false} and ~0ull
    w.x.push_back(mk<F>::zero()), w.y.push_back(mk<F>::zero()), w.index.push_back(0x7FFFFFFFFFFFFFFFull), w.rebase.push_back(0);
    w.rebases.push_back(~0ull);
    // InitResults(DontSaveForReuse, orbitX, orbitY, radius, fileProvidedIters - 1, 0), :2125-2134
    const uint64_t count = ref_it + 1; // m_UncompressedItersInOrbit
    ob.period = periodic ? ref_it + 1 : 0;
    ob.compressed = false;
    if constexpr (num<F>::is_plain) {
        using T = scalar_t<F>;
        // static_cast<T>(halfH.toDouble()), :2136-2137; toDouble = mantissa * getMultiplier(exp), HDRFloat.h:553-557
        ob.maxRadius = preal<T>{(T)(halfH.mantissa * multiplier<double>((int32_t)halfH.exp))};
        ob.orbitXLow = (T)mpf_get_d(ob.cx.v);                                    // T{orbitX}
        ob.orbitYLow = (T)mpf_get_d(ob.cy.v);
        decompress_max(w, preal<T>{ob.orbitXLow}, preal<T>{ob.orbitYLow}, count, ob.x, ob.y);
    } else {
        ob.maxRadius = hr_reduced(hreal<F>{(F)halfH.mantissa, (int32_t)halfH.exp});
        ob.orbitXLow = hr_from_mpf<F>(ob.cx.v);
        ob.orbitYLow = hr_from_mpf<F>(ob.cy.v);
        decompress_max(w, ob.orbitXLow, ob.orbitYLow, count, ob.x, ob.y);
        ob.bad.assign(ob.x.size(), 0);
    }
    return ob.x.size() == count;
}

} // namespace

extern "C" int fsh_orbit_save_im(const fsh_orbit *o, uint64_t num_iterations, int compression_exp, const char *path,
                                 int exp_bytes)
{
    return o->is64 ? save_im_orbit<double>(o->d, o->d.orbitXLow, o->d.orbitYLow, num_iterations, compression_exp, path, exp_bytes)
                   : save_im_orbit<float>(o->f, o->f.orbitXLow, o->f.orbitYLow, num_iterations, compression_exp, path, exp_bytes);
}

static fsh_orbit *orbit_load_im(FILE *f, uint64_t *iteration_limit);

extern "C" fsh_orbit *fsh_orbit_load_im(const char *path, uint64_t *iteration_limit)
{
    FILE *f = fopen(path, "rb");
    if (!f)
        return nullptr;
    // nothing may unwind through the C boundary (a corrupt file can still make a vector throw): NULL, like any other refusal
    fsh_orbit *out = nullptr;
    try {
        out = orbit_load_im(f, iteration_limit);
    } catch (...) {
        out = nullptr;
    }
    fclose(f);
    return out;
}

static fsh_orbit *orbit_load_im(FILE *f, uint64_t *iteration_limit)
{
    uint64_t header[4];
    ImHR hh;
    uint64_t limit = 0;
    std::unique_ptr<fsh_orbit> out;
    if (fread(header, 8, 4, f) == 4 && (header[0] == kImMagic || header[0] == kSharksMagic) && header[3] != 0 &&
        fseek(f, (long)header[2], SEEK_SET) == 0 && fread(&hh, sizeof(hh), 1, f) == 1 && fread(&limit, 8, 1, f) == 1) {
        // (a file is untrusted input: GMP aborts on an absurd precision, it does not throw -- the deepest view the renderer's
        // int32 exponents can express needs 2^31 bits)
        if (hh.exp < -(int64_t)kMaxImPrecisionBits)
            return nullptr;
        const uint64_t precision = (uint64_t)(-std::min<int64_t>(0, hh.exp)) + 120u;
        mpf_set_default_prec(precision);
        Mp X(precision, 0), Y(precision, 0);
        const long at = ftell(f);
        int width_ok = 0;
        for (int exp_bytes : {4, 8}) {
            fseek(f, at, SEEK_SET);
            if (im_read_mpf(f, X.v, exp_bytes) && im_read_mpf(f, Y.v, exp_bytes) && (uint64_t)ftell(f) == header[3]) {
                width_ok = exp_bytes;
                break;
            }
        }
        if (width_ok) {
            out = std::make_unique<fsh_orbit>();
            out->is64 = header[0] == kImMagic ? 1 : 0; // SubType double <-> Imagina's magic, float <-> "Sharks:)" (:3052-3058)
            bool ok;
            if (out->is64) {
                out->d.cx = X, out->d.cy = Y, out->d.prec_bits = precision;
                ok = load_im_orbit<double>(f, header[3], out->d, limit, ImHR{hh.mantissa, hh.exp});
            } else {
                out->f.cx = X, out->f.cy = Y, out->f.prec_bits = precision;
                ok = load_im_orbit<float>(f, header[3], out->f, limit, ImHR{hh.mantissa, hh.exp});
            }
            if (!ok)
                out.reset();
            else if (iteration_limit)
                *iteration_limit = limit;
        }
    }
    return out.release();
}

// ".im" files with a reference orbit for the non-ExtendedRange types (float: "Sharks:)" magic, double: Imagina's;
// ReferenceHeader::ExtendedRange = false; RefOrbitCalc.cpp:3039-3115 / :3386-3412, PerturbationResults.cpp:2047-2075, 2177-2183)
extern "C" int fsh_plain_save_im(const fsh_plain *h, uint64_t num_iterations, int compression_exp, const char *path, int exp_bytes)
{
    if (h->kind == 0)
        return save_im_orbit<plain<float>>(h->f.ob, preal<float>{h->f.ob.orbitXLow}, preal<float>{h->f.ob.orbitYLow},
                                           num_iterations, compression_exp, path, exp_bytes);
    return save_im_orbit<plain<double>>(h->d.ob, preal<double>{h->d.ob.orbitXLow}, preal<double>{h->d.ob.orbitYLow},
                                        num_iterations, compression_exp, path, exp_bytes);
}

static fsh_plain *plain_load_im(FILE *f, uint64_t *iteration_limit, int host_threads)
{
    uint64_t header[4];
    ImHR hh;
    uint64_t limit = 0;
    std::unique_ptr<fsh_plain> out;
    if (fread(header, 8, 4, f) == 4 && (header[0] == kImMagic || header[0] == kSharksMagic) && header[3] != 0 &&
        fseek(f, (long)header[2], SEEK_SET) == 0 && fread(&hh, sizeof(hh), 1, f) == 1 && fread(&limit, 8, 1, f) == 1) {
        // (untrusted input, as in orbit_load_im: bound the precision GMP is asked for)
        if (hh.exp < -(int64_t)kMaxImPrecisionBits)
            return nullptr;
        const uint64_t precision = (uint64_t)(-std::min<int64_t>(0, hh.exp)) + 120u;
        mpf_set_default_prec(precision);
        Mp X(precision, 0), Y(precision, 0);
        const long at = ftell(f);
        int width_ok = 0;
        for (int exp_bytes : {4, 8}) {
            fseek(f, at, SEEK_SET);
            if (im_read_mpf(f, X.v, exp_bytes) && im_read_mpf(f, Y.v, exp_bytes) && (uint64_t)ftell(f) == header[3]) {
                width_ok = exp_bytes;
                break;
            }
        }
        if (width_ok) {
            out = std::make_unique<fsh_plain>();
            out->kind = header[0] == kImMagic ? 1 : 0; // T double <-> Imagina's magic, float <-> "Sharks:)" (:3386-3412)
            bool ok;
            if (out->kind == 1) {
                out->d.ob.cx = X, out->d.ob.cy = Y;
                ok = load_im_orbit<plain<double>>(f, header[3], out->d.ob, limit, ImHR{hh.mantissa, hh.exp});
                if (ok)
                    out->d.finish(host_threads);
            } else {
                out->f.ob.cx = X, out->f.ob.cy = Y;
                ok = load_im_orbit<plain<float>>(f, header[3], out->f.ob, limit, ImHR{hh.mantissa, hh.exp});
                if (ok)
                    out->f.finish(host_threads);
            }
            if (!ok)
                out.reset();
            else if (iteration_limit)
                *iteration_limit = limit;
        }
    }
    return out.release();
}

extern "C" fsh_plain *fsh_plain_load_im(const char *path, uint64_t *iteration_limit, int host_threads)
{
    FILE *f = fopen(path, "rb");
    if (!f)
        return nullptr;
    fsh_plain *out = nullptr;
    try { // nothing may unwind through the C boundary
        out = plain_load_im(f, iteration_limit, host_threads);
    } catch (...) {
        out = nullptr;
    }
    fclose(f);
    return out;
}
