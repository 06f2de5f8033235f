// bla_table.cpp -- the BLA table of an HDRFloat orbit: BLAS<uint32_t, HDRFloat<F>>::Init, BLAS.cpp:25-255 with BLA<T> helpers
// BLA.cuh:7-110, through the level pyramid of inputs_state.hpp.
#include "inputs_state.hpp"

namespace {

// (BlaRec<F> and the record arithmetic: csrc/bla_math.hpp, shared with the device builder)

template <class F> struct BlaBuilder {
    std::vector<std::vector<BlaRec<F>>> B;
    int32_t LM2 = 0;

    BlaBuilder(const OrbitT<F> &ob, hreal<F> blaSize) // (BLAS::Init's blaSize: the reference passes GetMaxRadius())
    {
        const hreal<F> precision = hr_div(hr_from_number<F>(F(1)), hr_from_mant<F>(F(8388608))); // T(1)/T{1L<<23}
        // BLAS::CreateOneStep, BLAS.cpp:74-93, and BLAS::MergeTwoBlas, BLAS.cpp:25-47
        auto one_step = [&](size_t m) { return bla_one_step<F>(hc_from_hr(ob.x[m], ob.y[m]), precision); };
        auto merge = [&](const BlaRec<F> &x, const BlaRec<F> &y) { return bla_merge<F>(x, y, blaSize); };
        LM2 = bla_pyramid(ob.x.size(), B, one_step, merge); // BLAS::Init, BLAS.cpp:212-255
    }
};

// the table in the ABI's records (Rec = fs_bla_hdr32 / fs_bla_hdr64; their padding members are zeroed by the aggregate form)
template <class F, class Rec>
void pack_bla(const OrbitT<F> &ob, const void *bla_size, std::vector<std::vector<Rec>> &levels, fsh_bla &r)
{
    using Real = decltype(Rec::r2);
    const Real *given = (const Real *)bla_size;
    const BlaBuilder<F> b(ob, given ? hreal<F>{given->m, given->e} : ob.maxRadius);
    r.lm2 = b.LM2;
    levels.resize(b.B.size());
    for (size_t l = 0; l < b.B.size(); l++) {
        levels[l].resize(b.B[l].size());
        for (size_t k = 0; k < b.B[l].size(); k++) {
            const auto &s = b.B[l][k];
            auto R = [](hreal<F> h) { return Real{h.m, h.e}; };
            levels[l][k] = Rec{R(s.r2), R(s.Ax), R(s.Ay), R(s.Bx), R(s.By), s.l};
        }
    }
    bla_export(levels, r.ptrs, r.sizes);
}

} // namespace

// bla_size: NULL = the orbit's own maxRadius, else an fs_real_hdr32 / fs_real_hdr64 (the orbit's type) taken in its place
extern "C" fsh_bla *fsh_bla_create_ex(const fsh_orbit *o, const void *bla_size)
{
    auto r = std::make_unique<fsh_bla>();
    r->is64 = o->is64;
    if (!o->is64)
        pack_bla(o->f, bla_size, r->levels32, *r);
    else
        pack_bla(o->d, bla_size, r->levels64, *r);
    return r.release();
}
extern "C" fsh_bla *fsh_bla_create(const fsh_orbit *o) { return fsh_bla_create_ex(o, nullptr); }
extern "C" fsh_bla *fsh_bla_create_hdr32(const fsh_orbit *o) { return o->is64 ? nullptr : fsh_bla_create(o); }
extern "C" void fsh_bla_destroy(fsh_bla *b) { delete b; }
extern "C" int32_t fsh_bla_num_levels(const fsh_bla *b) { return (int32_t)b->ptrs.size(); }
extern "C" int32_t fsh_bla_lm2(const fsh_bla *b) { return b->lm2; }
extern "C" const void *const *fsh_bla_level_ptrs(const fsh_bla *b) { return b->ptrs.data(); }
extern "C" const uint64_t *fsh_bla_level_sizes(const fsh_bla *b) { return b->sizes.data(); }
