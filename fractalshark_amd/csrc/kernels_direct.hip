// kernels_direct.hip -- the direct (no reference orbit) escape-time kernels with a CPU twin: plain double and HDRFloat<float | double>
// (Fractal::CalcCpuHDR), their row-prefix kernels and launchers.  The low-precision direct kernels, which have none, are in
// kernels_direct_lp.hip.  Compiled with -ffp-contract=off (see hdr_math.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fs_layout.h"
#include "hdr_math.hpp"
#include "kernels.h"
#include "kernel_common.hpp"
#include "launch_dispatch.hpp"

using namespace fs;

// ------------------------------------------------------------------------------------------------
// Direct double-precision escape time.  CPU twin: Fractal::CalcCpuHDR<uint32_t,double,double>
// (Fractal.cpp:2148-2183): cy = maxY - dy*(double)(float)y; cx starts at minX and is ACCUMULATED (cx += dx)
// along the row, so a lane at column x replays x additions; z0 = c; bailout sum > 4.
// Replaces mandel_1x_double (FractalSharkGpuLib/LowPrecisionKernels.cuh:79-171).
template <bool kStats, class IterT = uint32_t>
__global__ void __launch_bounds__(256) k_direct_f64(FsDirectArgs64 A)
{
    const uint32_t X = blockIdx.x * 64u + (threadIdx.x & 63u);
    const uint32_t L = blockIdx.y * 4u + (threadIdx.x >> 6);
    uint64_t c_pt = 0, c_px = 0;
    const uint32_t Y = global_row(A.frame, L);
    const bool live = X < A.frame.width && L < A.frame.local_rows && Y < A.frame.height;
    if (live) {
        c_px = 1;
        // Row prefix of cx: minX + dx + dx + ... (X times), rounded after every addition like the CPU loop.
        // The prefix for the wave's first column comes from a table built once per frame (A.cx_row).
        const double cx = A.cx_row[X];
        const double cy = A.maxY - A.dy * (double)((float)Y);
        double zx = cx, zy = cy;
        const IterT n_iterations = iter_cap<IterT>(A.n_iterations, A.n_iterations_hi);
        IterT i;
        for (i = 0; i < n_iterations; i++) {
            const double zx2 = zx * zx;
            const double zy2 = zy * zy;
            const double sum = zx2 + zy2;
            if (sum > 4.0)
                break;
            zy = 2.0 * zx * zy;
            zx = zx2 - zy2;
            zx += cx;
            zy += cy;
        }
        if (kStats)
            c_pt = i;
        store_iter(A.out, A.frame, L, X, i);
    }
    if (kStats)
        add_stats(A.stats, 0, 0, c_pt, c_px);
}

// cx_row[x] = minX (+ dx) x times, sequentially rounded: a serial scan, done by one lane once per frame
// (W <= 61440 additions).
__global__ void k_direct_row_prefix_f64(double minX, double dx, uint32_t width, double *cx_row)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double cx = minX;
        for (uint32_t x = 0; x < width; x++) {
            cx_row[x] = cx;
            cx += dx;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Direct escape time in HDRFloat<F>.  CPU twin: Fractal::CalcCpuHDR<uint32_t,HDRFloat<F>,F> (Fractal.cpp:2148-2183;
// CpuHDR32 / CpuHDR64): z0 = c, bailout Reduce(zx^2+zy^2) > 4, zy = (2*zx)*zy, zx = zx2 - zy2, += c, Reduce both.
// cx is the CPU's accumulated `cx += dx` (un-reduced HDR adds) from a 1-lane serial scan, like k_direct_f64.
// Replaces mandel_hdr_float (FractalSharkGpuLib/LowPrecisionKernels.cuh:682-777).
template <class F, bool kStats, class IterT = uint32_t>
__global__ void __launch_bounds__(256) k_direct_hdr(FsDirectHdrArgsT<F> A)
{
    const uint32_t X = blockIdx.x * 64u + (threadIdx.x & 63u);
    const uint32_t L = blockIdx.y * 4u + (threadIdx.x >> 6);
    uint64_t c_pt = 0, c_px = 0;
    const uint32_t Y = global_row(A.frame, L);
    const bool live = X < A.frame.width && L < A.frame.local_rows && Y < A.frame.height;
    if (live) {
        c_px = 1;
        const hreal<F> cx = A.cx_row[X];
        // T{static_cast<float>(y)}: non-template HDRFloat(T mant) for float, templated (U = float) ctor for double
        const hreal<F> yh = sizeof(F) == 4 ? hr_from_mant<F>((F)(float)Y) : hr_from_number<F>((F)(float)Y);
        const hreal<F> cy = hr_sub(A.maxY, hr_mul(A.dy, yh));
        const hreal<F> Four{F(1), 2};
        const hreal<F> Two{F(1), 1};
        hreal<F> zx = cx, zy = cy;
        const IterT n_iterations = iter_cap<IterT>(A.n_iterations, A.n_iterations_hi);
        IterT i;
        for (i = 0; i < n_iterations; i++) {
            const hreal<F> zx2 = hr_mul(zx, zx);
            const hreal<F> zy2 = hr_mul(zy, zy);
            const hreal<F> sum = hr_reduced(hr_add(zx2, zy2));
            if (hr_cmp_pos(sum, Four) > 0)
                break;
            zy = hr_mul(hr_mul(Two, zx), zy);
            zx = hr_sub(zx2, zy2);
            zx = hr_add(zx, cx);
            zy = hr_add(zy, cy);
            hr_reduce(zx);
            hr_reduce(zy);
        }
        if (kStats)
            c_pt = i;
        store_iter(A.out, A.frame, L, X, i);
    }
    if (kStats)
        add_stats(A.stats, 0, 0, c_pt, c_px);
}

template <class F> __global__ void k_direct_row_prefix_hdr(hreal<F> minX, hreal<F> dx, uint32_t width, hreal<F> *cx_row)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hreal<F> cx = minX;
        for (uint32_t x = 0; x < width; x++) {
            cx_row[x] = cx;
            cx = hr_add(cx, dx);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Host-callable launchers (called from renderer_launch.cpp through kernels.h).
template <class F>
static void launch_direct_hdr(const FsDirectHdrArgsT<F> &A, hreal<F> minX, hreal<F> dx, bool stats, hipStream_t s)
{
    hipLaunchKernelGGL((k_direct_row_prefix_hdr<F>), dim3(1), dim3(64), 0, s, minX, dx, A.frame.width, A.cx_row);
    fsl::with_counting(A.frame, stats, [&](auto c) {
        using C = decltype(c);
        hipLaunchKernelGGL((k_direct_hdr<F, C::stats, typename C::Iter>), fsl::row_grid(A.frame), dim3(256), 0, s, A);
    });
}
void fsk_direct_hdr32(const FsDirectHdrArgsT<float> &A, hreal<float> minX, hreal<float> dx, bool stats, hipStream_t s)
{
    launch_direct_hdr<float>(A, minX, dx, stats, s);
}
void fsk_direct_hdr64(const FsDirectHdrArgsT<double> &A, hreal<double> minX, hreal<double> dx, bool stats, hipStream_t s)
{
    launch_direct_hdr<double>(A, minX, dx, stats, s);
}

void fsk_direct_f64(const FsDirectArgs64 &A, double minX, double dx, bool stats, hipStream_t s)
{
    hipLaunchKernelGGL(k_direct_row_prefix_f64, dim3(1), dim3(64), 0, s, minX, dx, A.frame.width, A.cx_row);
    fsl::with_counting(A.frame, stats, [&](auto c) {
        using C = decltype(c);
        hipLaunchKernelGGL((k_direct_f64<C::stats, typename C::Iter>), fsl::row_grid(A.frame), dim3(256), 0, s, A);
    });
}
