// feature_axes_ref.cpp -- the axes of fsh_feature_pt_axes combined per grid point: C(re, im), reduced (the host instantiation of
// hc_from_hr, hc_reduced of csrc/hdr_math.hpp), for tests/test_feature_map_cpu.py.  g++ -O2 -ffp-contract=off, as libfsinputs.
#include "../../fractalshark_amd/csrc/hdr_math.hpp"
#include "../../include/fs_layout.h"

using namespace fs;

namespace {

template <class F, class Real, class Cplx> void combine(const Real *re, uint32_t nx, const Real *im, uint32_t ny, Cplx *out)
{
    for (uint32_t gy = 0; gy < ny; ++gy)
        for (uint32_t gx = 0; gx < nx; ++gx) {
            const hcplx<F> c = hc_reduced(hc_from_hr(hreal<F>{re[gx].m, re[gx].e}, hreal<F>{im[gy].m, im[gy].e}));
            Cplx r{};
            r.re = c.re, r.im = c.im, r.e = c.e;
            out[(size_t)gy * nx + gx] = r;
        }
}

} // namespace

// out[gy * nx + gx] = C(re[gx], im[gy]) reduced: fs_cplx_hdr64 of fs_real_hdr64 axes when is64, else fs_cplx_hdr32 of fs_real_hdr32.
extern "C" void far_combine(int is64, const void *re, uint32_t nx, const void *im, uint32_t ny, void *out)
{
    if (is64)
        combine<double>((const fs_real_hdr64 *)re, nx, (const fs_real_hdr64 *)im, ny, (fs_cplx_hdr64 *)out);
    else
        combine<float>((const fs_real_hdr32 *)re, nx, (const fs_real_hdr32 *)im, ny, (fs_cplx_hdr32 *)out);
}
