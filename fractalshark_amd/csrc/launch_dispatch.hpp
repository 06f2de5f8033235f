// launch_dispatch.hpp -- host side of the kernel launchers (fsk_* in the kernels*.hip units): the launch geometry, and the few
// functions that turn a launcher's run-time switches into the template arguments of the instantiation it launches.
//
// Which instantiations exist -- the rule every family of iteration kernels follows:
//   * the mode (FS_MODE_FULL / PO / LAO) and every A/B switch of a family are template arguments: all their values are built;
//   * step counters (kStats) are built with 32-bit iteration counters only.  A launch that counts iterations in 64 bits
//     (FsFrame::wide: a cap of 2^32 and above, or the test switch) has no step-counting form, whatever fs_enable_step_count says:
//     with_counting() below has three answers, not four;
//   * a kernel on a waypoint-resident orbit (kSeq) has no step counters in either width.
// The host side says the same thing to its callers: fs_renderer::last_launch_wide makes fs_read_step_count refuse after such
// launches.
// Exceptions, built because tools and tests read them:
//   * the literal LAv2 kernel (k_lav2_lit, kernels_lav2_lit.hip) counts steps with 64-bit counters too, and with 32-bit ones on a
//     waypoint-resident orbit; only its <kSeq, uint64_t> form has none;
//   * the perturbation-only / BLA kernel (k_perturb_scalar, kernels_perturb.hip) counts steps with 64-bit counters too.
// A combination that is not built is never named by a launcher: it is clamped before the dispatch or left out with `if constexpr`.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernels.h"

namespace fsl {

// ---- geometry.  Workgroups are 256 threads = four waves.
// tile_pixel() (kernel_common.hpp): a wave renders an 8 x 8 tile, a workgroup four tiles side by side
inline dim3 tile_grid(uint32_t width, uint32_t rows) { return dim3((width + 31) / 32, (rows + 7) / 8, 1); }
inline dim3 tile_grid(const FsFrame &f) { return tile_grid(f.width, f.local_rows); }
// waves of a tile launch (fsk_tile_launch_waves for the host side): at least the frame's number of tiles
inline uint32_t tile_waves(const FsFrame &f)
{
    const dim3 g = tile_grid(f);
    return g.x * g.y * 4u;
}
// a wave renders 64 pixels of a row, a workgroup four rows
inline dim3 row_grid(const FsFrame &f) { return dim3((f.width + 63) / 64, (f.local_rows + 3) / 4, 1); }

// ---- dispatch: fn is a generic lambda and reads its argument's type, `decltype(m)::value` and the like
// fn(std::integral_constant<int, FS_MODE_*>)
template <class Fn> void with_mode(int mode, Fn &&fn)
{
    if (mode == FS_MODE_FULL)
        fn(std::integral_constant<int, FS_MODE_FULL>{});
    else if (mode == FS_MODE_PO)
        fn(std::integral_constant<int, FS_MODE_PO>{});
    else
        fn(std::integral_constant<int, FS_MODE_LAO>{});
}

// fn(std::bool_constant<b>)
template <class Fn> void with_bool(bool b, Fn &&fn)
{
    if (b)
        fn(std::true_type{});
    else
        fn(std::false_type{});
}

// the iteration counter of a launch: iter_t<FsFrame::wide != 0>
template <bool kWide> using iter_t = std::conditional_t<kWide, uint64_t, uint32_t>;

// fn(Counting<kStats, IterT>): the three pairs the rule above leaves
template <bool kStats, class IterT> struct Counting {
    static constexpr bool stats = kStats;
    using Iter = IterT;
};
template <class Fn> void with_counting(const FsFrame &f, bool stats, Fn &&fn)
{
    if (f.wide != 0u)
        fn(Counting<false, uint64_t>{});
    else if (stats)
        fn(Counting<true, uint32_t>{});
    else
        fn(Counting<false, uint32_t>{});
}

} // namespace fsl
