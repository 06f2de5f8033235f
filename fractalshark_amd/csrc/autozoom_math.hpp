// autozoom_math.hpp -- the FilamentTip score of fs_autozoom_pick, one text for the device (kernels_autozoom.hip: selects the
// candidates) and the host (renderer_analysis.cpp: decides among them with libm).  AutoZoomer.cpp:338-361, operation by operation; built
// with -ffp-contract=off.  Everything but log() is IEEE arithmetic (+ - * / sqrt, correctly rounded on both sides), so the two
// sides differ by what their log() functions differ.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace fs {

// max_dist = sqrt(double(W * W + H * H)) / 2.0, computed once by the host.
__host__ __device__ inline double az_tip_score(uint64_t cur, uint32_t high, uint32_t x, uint32_t y, uint32_t W, uint32_t H,
                                               uint64_t n_iterations, double avg, double max_dist)
{
    const double tipness = 1.0 - (double)high / 4.0;
    const double numerator = (double)cur - avg;
    const double denominator = (double)n_iterations - avg;
    const double raw = denominator > 0 ? log(1.0 + numerator) / log(1.0 + denominator) : 0.5;
    const double elevation = 1.0 - raw;
    const double ddx = (double)((int32_t)x - (int32_t)(W / 2u));
    const double ddy = (double)((int32_t)y - (int32_t)(H / 2u));
    const double dist = sqrt(ddx * ddx + ddy * ddy) / max_dist;
    return tipness * elevation * (0.3 + 0.7 * dist);
}

// Doubles (no NaN) <-> unsigned keys of the same order: an integer atomicMax on the key is a maximum of the doubles, whatever
// order the lanes arrive in.  Key 0 is below every double's key.
__host__ __device__ inline uint64_t az_key_of(double v)
{
    union {
        double d;
        uint64_t u;
    } c;
    c.d = v;
    return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}
__host__ __device__ inline double az_double_of(uint64_t key)
{
    union {
        double d;
        uint64_t u;
    } c;
    c.u = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
    return c.d;
}

} // namespace fs
