// renderer_launch.cpp -- the iteration kernels' launch paths (fs_render_*): argument blocks, the choice of kernel, the recorded
// pixel / tile orders of repeated frames, and the switches and counters that belong to a launch.
#include "renderer_state.hpp"

#include <cmath>
#include <cstdlib>

using namespace fsr;

namespace {

FsFrame make_frame(const fs_renderer *r)
{
    FsFrame f;
    f.width = r->width;
    f.height = r->height;
    f.rounded_width = r->w_block * 16u;
    f.local_rows = r->local_rows;
    f.band_first = r->band_first;
    f.band_rows = r->band_rows;
    f.band_stride = r->band_stride;
    f.iter_u64 = r->iter_bytes == 8 ? 1u : 0u;
    f.wide = (r->variant & FS_VARIANT_FLAG_WIDE) != 0 ? 1u : 0u; // (|= cap >= 2^32 where the cap is known)
    return f;
}

// "long tiles first" (fs_render_bla, perturbation only): the probe runs each tile's centre pixel for n_iterations /
// kTileProbeDivisor steps; on by default for an iteration limit far above the bulk of a frame's pixels and enough tiles
// for an order to matter
constexpr uint64_t kTileProbeDivisor = 32;
constexpr uint64_t kTileOrderMinIterations = 1ull << 18;
constexpr uint32_t kTileOrderMinTiles = 4096;
// the same for the self-recorded order of the tuned LAv2 kernel: below this many tiles the chip is not full anyway
constexpr uint32_t kLav2OrderMinTiles = 2048;

} // namespace

static void fill_coords(FsCoordsT<float> &c, const void *coords)
{
    const fs_real_hdr32 *p = (const fs_real_hdr32 *)coords;
    c.dx = fs::hreal32{p[0].m, p[0].e};
    c.dy = fs::hreal32{p[1].m, p[1].e};
    c.centerX = fs::hreal32{p[2].m, p[2].e};
    c.centerY = fs::hreal32{p[3].m, p[3].e};
}
static void fill_coords(FsCoordsT<double> &c, const void *coords)
{
    const fs_real_hdr64 *p = (const fs_real_hdr64 *)coords;
    c.dx = fs::hreal64{p[0].m, p[0].e};
    c.dy = fs::hreal64{p[1].m, p[1].e};
    c.centerX = fs::hreal64{p[2].m, p[2].e};
    c.centerY = fs::hreal64{p[3].m, p[3].e};
}

// What every launch-argument block of kernels.h starts with: the iteration buffer, the statistics words, the frame, and the
// iteration cap in two halves -- a cap of 2^32 and more selects the 64-bit counting instantiation of the kernel.
template <class Args> static void init_args(fs_renderer *r, Args &A, uint64_t n_iterations)
{
    memset(&A, 0, sizeof(A));
    A.out = (uint32_t *)r->iters();
    A.stats = r->stats;
    A.frame = make_frame(r);
    A.n_iterations = (uint32_t)n_iterations;
    A.n_iterations_hi = (uint32_t)(n_iterations >> 32);
    A.frame.wide |= A.n_iterations_hi != 0u ? 1u : 0u;
    r->last_launch_wide = A.frame.wide != 0u;
}

template <class F> static void fill_lav2(fs_renderer *r, FsLav2ArgsT<F> &A, const void *coords, uint64_t n_iterations, int parity)
{
    init_args(r, A, n_iterations);
    A.las = r->las.as<const typename FsDev<F>::LA>();
    A.stages = r->stages.as<fs_la_stage_u32>();
    fill_coords(A.coords, coords);
    A.orbit_count = (uint32_t)r->orbit_uncompressed;
    A.period = (uint32_t)r->orbit_period;
    A.stage_count = r->n_stages;
    A.la_valid = r->la_ok ? r->la_valid : 0;
    A.use_at = r->use_at;
    A.parity = (parity == FS_PARITY_CPU_GPUSTAGE) ? FS_PARITY_GPUSTAGE : FS_PARITY_LITERAL;
    A.orbit_count_hi = (uint32_t)(r->orbit_uncompressed >> 32);
    A.period_hi = (uint32_t)(r->orbit_period >> 32);
    A.at_step_hi = r->at_step_hi;
    A.la_u64 = r->la_u64 ? 1u : 0u;
}

// How every fs_render_* begins.  kNoFrame: return *rc now -- the HIP error of a device that cannot be selected, else 0: there is
// nothing to render into (no fs_init_memory yet, as GPU_Render.cu:626-628, 1007-1009, 1317-1319; or a renderer that owns no
// row of the frame, a rank beyond the last band).  kRefused: *rc says what is wrong with the call.
enum class Begin { kGo, kNoFrame, kRefused };

static Begin render_begin(fs_renderer *r, bool type_ok, uint64_t n_iterations, uint32_t *rc)
{
    *rc = use_device(r);
    if (*rc != 0u || !r->memory_initialized() || r->local_rows == 0)
        return Begin::kNoFrame;
    if (!type_ok)
        *rc = FS_ERR_UNSUPPORTED;
    else if (n_iterations > 0xFFFFFFFFull && r->iter_bytes != 8)
        *rc = (uint32_t)hipErrorInvalidValue; // a 4-byte IterType cannot hold such a count
    if (*rc == 0u)
        exact_drop_kept(r); // (the frame the exact renderer's kept set describes is about to be replaced)
    return *rc != 0u ? Begin::kRefused : Begin::kGo;
}

static int kernel_mode(int lav2_mode)
{
    return lav2_mode == FS_LAV2_FULL ? FS_MODE_FULL : (lav2_mode == FS_LAV2_PO ? FS_MODE_PO : FS_MODE_LAO);
}

// Pixel order for the LAv2 kernels that wait for their slowest lane (see kernels_order.hip).  pix_order_for: the order to launch
// this frame with, or nullptr (first frame of a view, small frames, 64-bit buffers, A/B switch, no memory); pix_order_after: called
// behind the frame's kernel when it ran WITHOUT an order -- sorts the buffer it has just written and keeps the result for the next
// frame with the same key.  Frames of fewer than kPixOrderMinPixels elements are not worth the sort.
constexpr uint64_t kPixOrderMinPixels = 1u << 20;

static fs_renderer::PixKey pix_key_of(fs_renderer *r, const FsFrame &f, int type_tag, int mode, int parity, const void *coords,
                                      size_t coords_bytes, uint64_t n_iterations)
{
    fs_renderer::PixKey k;
    memset(&k, 0, sizeof(k));
    k.rounded_width = f.rounded_width, k.local_rows = f.local_rows, k.band_first = f.band_first, k.band_rows = f.band_rows;
    k.band_stride = f.band_stride, k.type_tag = type_tag, k.mode = mode, k.parity = parity;
    k.orbit_gen = r->orbit_gen, k.orbit_epoch = r->orbit_epoch, k.n_iterations = n_iterations;
    memcpy(k.coords, coords, coords_bytes < sizeof(k.coords) ? coords_bytes : sizeof(k.coords));
    return k;
}

// elements of the iteration buffer of a frame, padding included
static uint64_t buffer_elems(const FsFrame &f) { return (uint64_t)f.rounded_width * ((f.local_rows + 7u) & ~7u); }

static bool pix_order_wanted(fs_renderer *r, const FsFrame &f)
{
    const uint64_t n = buffer_elems(f);
    // (FSMI355_STATS_KEEP_ORDER=1: a counting launch keeps the recorded order -- tools/c4_arm_probe.py counts what the ORDERED waves do)
    static const bool stats_keep = [] { const char *e = getenv("FSMI355_STATS_KEEP_ORDER"); return e && e[0] == '1'; }();
    return r->iter_bytes == 4 && f.wide == 0u && (!r->stats_on || stats_keep) && n >= kPixOrderMinPixels && n < 0x7FFFFFFFull &&
           (r->variant & FS_VARIANT_FLAG_NATURAL_ORDER) == 0 && (r->variant & FS_VARIANT_BASE_MASK) == FS_VARIANT_TUNED;
}

static const uint32_t *pix_order_for(fs_renderer *r, const FsFrame &f, const fs_renderer::PixKey &key)
{
    r->last_frame_ordered = false;
    if (!pix_order_wanted(r, f) || !r->pix_valid || !(r->pix_key == key))
        return nullptr;
    r->last_frame_ordered = true;
    return r->pix_order.as<uint32_t>();
}

// An order costs a sort (two for HDRFloat<double>) and is worth it only for a view that is rendered again: a viewer that zooms
// changes the coordinates with every frame and would pay for sorts it never uses.  So the first unordered frame of a key only
// leaves its key behind; the second one records and sorts; the third and later ones run ordered.  Returns whether THIS unordered
// frame is such a second one.
static bool pix_second_sighting(fs_renderer *r, const FsFrame &f, const fs_renderer::PixKey &key)
{
    const bool wanted = pix_order_wanted(r, f);
    const bool again = wanted && r->pix_seen && r->pix_seen_key == key;
    r->pix_seen = wanted;
    r->pix_seen_key = key;
    return again;
}

// The cost record of a frame that runs WITHOUT an order (the first of a view): a zeroed buffer in the iteration buffer's geometry
// that the kernel fills pixel by pixel (padding stays 0 and sorts last), or nullptr (no order wanted, no memory).
static uint32_t *pix_cost_for(fs_renderer *r, const FsFrame &f, bool frame_is_ordered)
{
    if (frame_is_ordered || !pix_order_wanted(r, f))
        return nullptr;
    const size_t bytes = (size_t)buffer_elems(f) * sizeof(uint32_t);
    if (buf_reserve(r, r->pix_cost, bytes, kFrame) != hipSuccess ||
        hipMemsetAsync(r->pix_cost.p, 0, bytes, r->compute) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return r->pix_cost.as<uint32_t>();
}

static void pix_order_after(fs_renderer *r, const FsFrame &f, const fs_renderer::PixKey &key, bool frame_was_ordered,
                            const uint32_t *cost = nullptr)
{
    if (frame_was_ordered || !pix_order_wanted(r, f))
        return; // (an ordered frame's buffer equals the one the order was made from: nothing new to learn)
    const uint32_t n = (uint32_t)buffer_elems(f);
    r->pix_valid = false;
    // the order, the sort's work memory and its temporary storage; sorted by the cost the frame recorded (round 5) -- or,
    // without a record, by the counts as before.  No memory: frames keep the tile mapping.
    if (buf_reserve(r, {{&r->pix_order, (size_t)n * sizeof(uint32_t)}, {&r->pix_work, (size_t)n * 2 * sizeof(uint32_t)},
                        {&r->pix_temp, fsk_pixel_order_temp_bytes(n)}}, kFrame, &r->pix_valid) != hipSuccess ||
        fsk_pixel_order_build(cost ? cost : (const uint32_t *)r->iters(), n, r->pix_work.as<uint32_t>(), r->pix_order.as<uint32_t>(),
                              r->pix_temp.p, r->pix_temp.cap, r->compute) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    r->pix_key = key;
    r->pix_valid = true;
}

// The tile order of a view's first frame (kernels_tile_sample.hip): S carries the frame, the coordinates and the AT record's values in
// binary64; -> order[n_slots] on the device (wave w of the frame's launch renders tile order[w]), or nullptr: not wanted (small frames,
// 64-bit buffers, A/B switch FSMI355_COLD_TILE_ORDER=0, FS_VARIANT_NATURAL_TILE_ORDER), no memory.  Queued on the compute stream.
static const uint32_t *cold_tile_order(fs_renderer *r, FsTileSampleArgs &S)
{
    static const bool off = [] { const char *e = getenv("FSMI355_COLD_TILE_ORDER"); return e && e[0] == '0'; }();
    if (off || !pix_order_wanted(r, S.frame) || S.StepLength == 0u)
        return nullptr;
    S.tiles_x = (S.frame.width + 7u) / 8u, S.tiles_y = (S.frame.local_rows + 7u) / 8u;
    S.n_slots = fsk_tile_launch_waves(S.frame);
    const size_t words = (size_t)S.n_slots * sizeof(uint32_t);
    if (buf_reserve(r, {{&r->cold_cost, words}, {&r->cold_order, words}, {&r->cold_work, 2 * words},
                        {&r->cold_temp, fsk_pixel_order_temp_bytes(S.n_slots)}}, kFrame) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    S.cost = r->cold_cost.as<uint32_t>();
    fsk_at_tile_sample64(S, r->compute);
    if (fsk_pixel_order_build(S.cost, S.n_slots, r->cold_work.as<uint32_t>(), r->cold_order.as<uint32_t>(), r->cold_temp.p,
                              r->cold_temp.cap, r->compute) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    fsk_tile_order_finish(r->cold_order.as<uint32_t>(), S.n_slots, S.tiles_x * S.tiles_y, r->compute);
    r->last_cold_ordered = true;
    return r->cold_order.as<uint32_t>();
}

// What cold_tile_order samples with; each caller converts its own AT record (head + tail, or mantissa and exponent).
static void fill_tile_sample(FsTileSampleArgs &S, const FsFrame &frame, const FsCoordsT<double> &coords, uint32_t n_iterations,
                             uint32_t step_length, fs::hreal<double> ThresholdC, fs::hreal<double> SqrEscapeRadius,
                             fs::hcplx<double> RefC, fs::hcplx<double> CCoeff)
{
    memset(&S, 0, sizeof(S));
    S.frame = frame;
    S.coords = coords;
    S.ThresholdC = ThresholdC, S.SqrEscapeRadius = SqrEscapeRadius;
    S.RefC = RefC, S.CCoeff = CCoeff;
    S.StepLength = step_length, S.n_iterations = n_iterations;
}

// ---- The launch paths of fs_render_lav2, which validates the call and picks one.

// The orbit is resident as waypoints only (fs_set_compressed_orbit_mode 1): the literal kernel with a sequential
// decompression cursor per pixel.
static uint32_t lav2_seq(fs_renderer *r, int type_tag, int mode, int parity, const void *coords, uint64_t n_iterations, bool wide)
{
    // 64-bit POSITIONS (and counters) whenever something does not fit 32 bits: the orbit's uncompressed length or period,
    // a table kept in the uint64_t layout -- besides the iteration cap and the test switch
    const bool wide_pos = wide || r->la_u64 || r->orbit_uncompressed > 0xFFFFFFFFull || r->orbit_period > 0xFFFFFFFFull;
    TimedLaunch t(r);
    auto launch = [&](auto f, const auto &at, const auto &c_low) { // f: 0.0f or 0.0, the float type of the orbit
        using F = decltype(f);
        FsLav2ArgsT<F> A;
        fill_lav2<F>(r, A, coords, n_iterations, parity);
        A.frame.wide |= wide_pos ? 1u : 0u;
        r->last_launch_wide = A.frame.wide != 0u;
        A.at = at;
        A.wp = r->wp_raw, A.n_wp = (uint32_t)r->orbit_size;
        A.cxLow = c_low[0], A.cyLow = c_low[1];
        fsk_lav2_seq(A, kernel_mode(mode), r->stats_on, r->compute);
    };
    if (type_tag == FS_T_HDR32)
        launch(0.0f, r->at, r->c_low32);
    else
        launch(0.0, r->at64, r->c_low64);
    return (uint32_t)hipGetLastError();
}

// the prepared HDRFloat<float> orbit and the companions of the tuned loops (FsLav2ArgsT<float> or FsBlaArgsT<float>)
template <class Args> static void set_orbit_hdr32(const fs_renderer *r, Args &A)
{
    A.zref = r->zref;
    A.zq = r->zq;
    A.zs = r->zq + r->zq_n;
    A.zs2 = r->zs2;
    A.zqb = r->zqb;
    A.znz = r->znz;
}

// GPURenderer::RenderPerturbLAv2<uint64_t, ...> with a cap the 32-bit counters cannot hold: the literal kernel
// instantiated with 64-bit counters (all three modes; the reference's arithmetic, operation by operation)
static uint32_t lav2_wide(fs_renderer *r, int type_tag, int mode, int parity, const void *coords, uint64_t n_iterations)
{
    TimedLaunch t(r);
    if (type_tag == FS_T_HDR32) {
        FsLav2ArgsT<float> A;
        fill_lav2<float>(r, A, coords, n_iterations, parity);
        set_orbit_hdr32(r, A);
        A.at = r->at;
        fsk_lav2_wide(A, kernel_mode(mode), r->stats_on, r->compute);
    } else {
        FsLav2ArgsT<double> A;
        fill_lav2<double>(r, A, coords, n_iterations, parity);
        A.zref = r->zref64;
        A.at = r->at64;
        fsk_lav2_wide(A, kernel_mode(mode), r->stats_on, r->compute);
    }
    return (uint32_t)hipGetLastError();
}

// Gpu1x32 / Gpu1x64 / Gpu2x32 PerturbedLAv2*: no CPU RenderAlgorithm exists for LAv2 on a plain type, the kernel
// restates the reference's CUDA kernel and ignores `parity`.  coords = float[4] / double[4] / fs_real_p2x32[4].
static uint32_t lav2_plain(fs_renderer *r, int type_tag, int mode, const void *coords, uint64_t n_iterations)
{
    FsLav2ArgsPlain A;
    init_args(r, A, n_iterations);
    // (the waypoint-resident instantiations are built without the step counters too: fs_read_step_count must refuse, not
    // report zeros)
    r->last_launch_wide = A.frame.wide != 0u || r->orbit_seq;
    A.las = r->las.p;
    A.stages = r->stages.as<fs_la_stage_u32>();
    memcpy(A.coords, coords, type_tag == FS_T_F32 ? 4 * sizeof(float) : 4 * sizeof(double));
    memcpy(A.at, r->at_plain, sizeof(A.at));
    A.orbit_count = (uint32_t)r->orbit_uncompressed;
    A.stage_count = r->n_stages;
    A.la_valid = (r->la_ok && r->la_type == type_tag) ? r->la_valid : 0;
    A.use_at = r->use_at;
    if (r->orbit_seq) { // waypoint-resident orbit: a cursor per pixel (k_lav2_plain<.., kSeq>)
        A.wp = r->wp_raw;
        A.n_wp = (uint32_t)r->orbit_size;
        memcpy(A.c_low[0], r->c_low_plain[0], 8);
        memcpy(A.c_low[1], r->c_low_plain[1], 8);
    } else {
        A.orbit = type_tag == FS_T_F64 ? (const void *)r->orbit_f64 : (const void *)r->orbit_plain;
    }
    TimedLaunch t(r);
    fsk_lav2_plain(A, type_tag == FS_T_F32 ? 0 : (type_tag == FS_T_F64 ? 1 : 2), kernel_mode(mode), r->stats_on, r->compute);
    return (uint32_t)hipGetLastError();
}

// HDRFloat<CudaDblflt>.  No CPU RenderAlgorithm exists for this type: the kernel restates the reference's CUDA kernel and
// ignores `parity` (coords are fs_real_2x32[4]).
static uint32_t lav2_2x32(fs_renderer *r, int mode, const void *coords, uint64_t n_iterations)
{
    FsLav2Args2x32 A;
    init_args(r, A, n_iterations);
    r->last_launch_wide = A.frame.wide != 0u || r->orbit_seq; // (kSeq: no counters either)
    A.las = r->las.as<const fs_la_2x32_u32>();
    A.stages = r->stages.as<fs_la_stage_u32>();
    memcpy(A.coords, coords, sizeof(A.coords));
    A.at = r->at2x32;
    A.orbit_count = (uint32_t)r->orbit_uncompressed;
    A.stage_count = r->n_stages;
    A.la_valid = (r->la_ok && r->la_type == FS_T_HDR2X32) ? r->la_valid : 0;
    A.use_at = r->use_at;
    if (r->orbit_seq) { // waypoint-resident orbit: a cursor per pixel (k_lav2_2x32<.., kSeq>)
        A.wp = (const fs_orbit_2x32_rc *)r->wp_raw;
        A.n_wp = (uint32_t)r->orbit_size;
        memcpy(&A.cxLow, r->c_low_plain[0], sizeof(fs_real_2x32));
        memcpy(&A.cyLow, r->c_low_plain[1], sizeof(fs_real_2x32));
    } else {
        A.orbit = r->orbit_2x32;
    }
    const fs_renderer::PixKey pk = pix_key_of(r, A.frame, FS_T_HDR2X32, mode, 0, coords, sizeof(A.coords), n_iterations);
    A.pixel_order = r->orbit_seq ? nullptr : pix_order_for(r, A.frame, pk);
    const bool second = !r->orbit_seq && A.pixel_order == nullptr && pix_second_sighting(r, A.frame, pk);
    A.pixel_cost = second ? pix_cost_for(r, A.frame, false) : nullptr;
    {
        TimedLaunch t(r);
        if (!r->orbit_seq && A.pixel_order == nullptr && !second && mode != FS_LAV2_PO && A.use_at && A.la_valid) {
            // a view's first frame: tiles in the order of a sampled PerformAT count (the record's values in binary64: head + tail, exact)
            auto R = [](const fs_real_2x32 &x) { return fs::hreal<double>{(double)x.head + (double)x.tail, x.e}; };
            auto Cx = [](const fs_cplx_2x32 &c) {
                return fs::hcplx<double>{(double)c.re_head + (double)c.re_tail, (double)c.im_head + (double)c.im_tail, c.e};
            };
            FsTileSampleArgs S;
            fill_tile_sample(S, A.frame, FsCoordsT<double>{R(A.coords[0]), R(A.coords[1]), R(A.coords[2]), R(A.coords[3])},
                             A.n_iterations, A.at.StepLength, R(A.at.ThresholdC), R(A.at.SqrEscapeRadius), Cx(A.at.RefC),
                             Cx(A.at.CCoeff));
            A.tile_order = cold_tile_order(r, S);
            A.tiles_x = S.tiles_x;
        }
        fsk_lav2_2x32(A, kernel_mode(mode), r->stats_on, r->compute);
    }
    if (second)
        pix_order_after(r, A.frame, pk, false, A.pixel_cost);
    return (uint32_t)hipGetLastError();
}

static uint32_t lav2_hdr32(fs_renderer *r, int mode, int parity, const void *coords, uint64_t n_iterations)
{
    FsLav2ArgsT<float> A;
    fill_lav2<float>(r, A, coords, n_iterations, parity);
    set_orbit_hdr32(r, A);
    A.at = r->at;
    // Longest tiles first, self-recorded.  Every frame of the tuned kernel stores one cost word per 8 x 8 tile (its
    // longest lane's step count); the NEXT frame of the same geometry, band layout and orbit generation is launched in
    // descending cost order (64 classes, raster order inside a class).  A frame ends one long wave after its last wave
    // was dispatched and the waves differ 2.5x in length, so the drain at the end of the launch shrinks from the longest
    // wave's duration towards the shortest's.  Which wave renders which tile changes no pixel; the first frame (and
    // every frame after fs_forget_tile_costs, or with FS_VARIANT_NATURAL_TILE_ORDER) runs in natural order.
    const uint32_t tiles_x = (r->width + 7u) / 8u, tiles_y = (r->local_rows + 7u) / 8u;
    const uint32_t n_tiles = tiles_x * tiles_y;
    const uint32_t n_slots = fsk_tile_launch_waves(A.frame);
    const bool tuned = (r->variant & FS_VARIANT_BASE_MASK) != FS_VARIANT_LITERAL;
    const bool record = tuned && n_tiles >= kLav2OrderMinTiles && (r->variant & FS_VARIANT_FLAG_NATURAL_ORDER) == 0;
    if (record) {
        FS_TRY(buf_reserve(r, {{&r->lav2_cost, (size_t)n_tiles * sizeof(uint32_t)},
                               {&r->lav2_sort_tmp, (size_t)fsk_tile_order_work_words(n_tiles) * sizeof(uint32_t)}},
                           kFrame, &r->lav2_cost_valid));
        FS_TRY(buf_reserve(r, r->lav2_order, ((size_t)n_slots + 1) * sizeof(uint32_t), kFrame));
        const fs_renderer::CostKey key{r->width, r->local_rows, A.frame.band_first, A.frame.band_rows,
                                       A.frame.band_stride, r->orbit_gen};
        A.tile_cost = r->lav2_cost.as<uint32_t>();
        A.tiles_x = tiles_x;
        if (r->lav2_cost_valid && r->lav2_cost_key == key)
            A.tile_order = r->lav2_order.as<uint32_t>();
        r->lav2_cost_key = key;
    }
    if (A.tile_order) {
        fsk_tile_order_by_cost(A.tile_cost, n_tiles, r->lav2_sort_tmp.as<uint32_t>(), r->lav2_order.as<uint32_t>(), n_slots,
                               r->compute);
        r->last_frame_ordered = true;
        r->lav2_last_ordered = true;
    }
    TimedLaunch t(r);
    fsk_lav2_hdr32(A, kernel_mode(mode), r->stats_on, r->variant, r->compute);
    r->lav2_cost_valid = record;
    return (uint32_t)hipGetLastError();
}

static uint32_t lav2_hdr64(fs_renderer *r, int mode, int parity, const void *coords, uint64_t n_iterations)
{
    FsLav2ArgsT<double> A;
    fill_lav2<double>(r, A, coords, n_iterations, parity);
    A.zref = r->zref64;
    A.at = r->at64;
    const fs_renderer::PixKey pk = pix_key_of(r, A.frame, FS_T_HDR64, mode, parity, coords, 4 * sizeof(fs_real_hdr64), n_iterations);
    A.pixel_order = pix_order_for(r, A.frame, pk);
    // PerformAT in a pass of its own, in the order of the AT iterations every pixel needs by itself (recorded by the view's
    // first frame): the AT loop reads no memory, so its waves can be made of pixels from anywhere -- equal work per wave --
    // while the frame's kernel keeps the order that keeps neighbours together (below).  A view's first frame has no such pass:
    // without an order its waves wait for their slowest pixel just as the kernel's do.
    const bool second = A.pixel_order == nullptr && pix_second_sighting(r, A.frame, pk);
    bool at_split = mode != FS_LAV2_PO && A.use_at && A.la_valid && pix_order_wanted(r, A.frame) &&
                    (A.pixel_order != nullptr || second);
    const uint32_t n_buf = (uint32_t)buffer_elems(A.frame); // (below 2^31 wherever an order is wanted)
    if (at_split &&
        buf_reserve(r, {{&r->at_res, n_buf * sizeof(FsAtRes)}, {&r->at_cost, n_buf * sizeof(uint32_t)},
                        {&r->at_order, n_buf * sizeof(uint32_t)}}, kFrame, &r->at_order_valid) != hipSuccess) {
        (void)hipGetLastError(); // no memory for it: PerformAT stays inside the frame's kernel
        at_split = false;
    }
    // (the AT order has a key of its own: it is a permutation of the buffer it was recorded on, and pix_order can be rebuilt
    // -- other row bands, a table without AT in between -- without it)
    const bool at_warm = at_split && r->at_order_valid && r->at_key == pk;
    const bool at_record = at_split && !at_warm; // (a view's first frame records nothing: a viewer that zooms never uses it)
    {
        TimedLaunch t(r);
        if (at_split) {
            FsLav2ArgsT<double> P = A;
            P.at_res = r->at_res.as<FsAtRes>();
            P.pixel_order = at_warm ? r->at_order.as<uint32_t>() : nullptr;
            if (at_record) {
                P.at_cost = r->at_cost.as<uint32_t>();
                FS_TRY(hipMemsetAsync(P.at_cost, 0, n_buf * sizeof(uint32_t), r->compute));
                r->at_order_valid = false;
            }
            fsk_at_pass64(P, r->compute);
            t.mid();
            A.at_res = P.at_res;
        }
        if (A.pixel_order == nullptr && !second && !at_split && mode != FS_LAV2_PO && A.use_at && A.la_valid) {
            // a view's first frame: tiles in the order of a sampled PerformAT count (kernels_tile_sample.hip)
            FsTileSampleArgs S;
            fill_tile_sample(S, A.frame, A.coords, A.n_iterations, A.at.StepLength,
                             fs::hreal<double>{A.at.ThresholdC.m, A.at.ThresholdC.e},
                             fs::hreal<double>{A.at.SqrEscapeRadius.m, A.at.SqrEscapeRadius.e},
                             fs::hcplx<double>{A.at.RefC.re, A.at.RefC.im, A.at.RefC.e},
                             fs::hcplx<double>{A.at.CCoeff.re, A.at.CCoeff.im, A.at.CCoeff.e});
            A.tile_order = cold_tile_order(r, S);
            A.tiles_x = S.tiles_x;
        }
        // the production kernel (kernels_hdr64.hip); FS_VARIANT_LITERAL keeps the operation-by-operation one for A/B
        // (k_lav2_hdr64 addresses its records with 32-bit byte offsets: an orbit or a table of 4 GB and more stays with the literal kernel)
        const bool small = (uint64_t)A.orbit_count * sizeof(FsZ64) < 0xFFFFFF00ull &&
                           (uint64_t)r->n_las * sizeof(fs_la_hdr64_u32) < 0xFFFFFF00ull;
        if (!small || (r->variant & FS_VARIANT_BASE_MASK) == FS_VARIANT_LITERAL)
            fsk_lav2_hdr64(A, kernel_mode(mode), r->stats_on, r->compute);
        else
            fsk_lav2_hdr64_fast(A, kernel_mode(mode), r->stats_on, r->compute);
    }
    // (sorted by COUNT, not by a recorded cost as the 2x32 frames are: this kernel's steps are cheap enough for the loads of
    // a wave whose lanes are scattered over the frame to cost more than the idle lanes they save -- 81 ms with the cost as
    // the key, 68 with its binades, 53 with the counts, which keep the pixels inside the set side by side: DESIGN.md 7)
    if (second)
        pix_order_after(r, A.frame, pk, false);
    if (at_record && r->pix_valid && r->pix_work.cap >= (size_t)n_buf * 2 * sizeof(uint32_t)) {
        // the AT pass's own order, from the costs it has just recorded (the sort's work memory is the pixel order's)
        if (fsk_pixel_order_build(r->at_cost.as<uint32_t>(), n_buf, r->pix_work.as<uint32_t>(), r->at_order.as<uint32_t>(),
                                  r->pix_temp.p, r->pix_temp.cap, r->compute) == hipSuccess) {
            r->at_order_valid = true;
            r->at_key = pk;
        } else
            (void)hipGetLastError();
    }
    return (uint32_t)hipGetLastError();
}

extern "C" {

uint32_t fs_render_bla(fs_renderer *r, int type_tag, const void *coords, uint64_t n_iterations)
{
    uint32_t rc;
    if (render_begin(r, type_tag == FS_T_HDR32 || type_tag == FS_T_HDR64 || type_tag == FS_T_F64, n_iterations, &rc) != Begin::kGo)
        return rc;
    if (!r->orbit_ok || r->orbit_type != type_tag)
        return FS_ERR_6;
    if (r->orbit_seq)
        return FS_ERR_UNSUPPORTED; // needs the expanded orbit (fs_set_compressed_orbit_mode 0)
    const bool use_bla = r->bla_n_levels > 2 && r->bla_levels_dev != nullptr && r->bla_type == type_tag;
    if (type_tag == FS_T_F64) {
        const double *c = (const double *)coords;
        FsBlaArgsF64 A;
        init_args(r, A, n_iterations);
        A.orbit = r->orbit_f64;
        A.levels = (const fs_bla_f64 *const *)r->bla_levels_dev;
        A.dx = c[0];
        A.dy = c[1];
        A.centerX = c[2];
        A.centerY = c[3];
        A.orbit_count = (uint32_t)r->orbit_uncompressed;
        A.lm2 = r->bla_lm2;
        TimedLaunch t(r);
        fsk_perturb_bla_f64(A, use_bla, r->stats_on, r->compute);
    } else if (type_tag == FS_T_HDR32) {
        FsBlaArgsT<float> A;
        init_args(r, A, n_iterations);
        set_orbit_hdr32(r, A);
        A.levels = (const fs_bla_hdr32 *const *)r->bla_levels_dev;
        A.queue = r->queue;
        fill_coords(A.coords, coords);
        A.orbit_count = (uint32_t)r->orbit_uncompressed;
        A.lm2 = r->bla_lm2;
        if (use_bla && r->bla_native_stale)
            if (uint32_t e = bla_make_native(r, r->bla_n_levels))
                return e;
        if (use_bla && r->bla_native_ok) {
            A.nrec = (const FsBlaRec *)(r->bla_native.as<const char>() + 256);
            A.nlad = (const int4 *)((const char *)A.nrec + (size_t)r->bla_native_total * sizeof(FsBlaRec));
            A.nkmax = (const long long *)(A.nlad + 2 * (size_t)r->bla_native_total);
            memcpy(A.level_off, r->bla_level_off, sizeof(A.level_off));
            if (r->bla_heap_ok) {
                A.hrec = r->bla_heap.as<const FsBlaRec>();
                A.hlad = (const int4 *)(A.hrec + r->bla_heap_positions);
                A.hq = A.hlad + 2 * (size_t)r->bla_heap_positions;
                A.zb = (const float4 *)(A.hq + 3 * (size_t)r->bla_heap_nq);
            }
        }
        // Long tiles first.  A perturbation-only frame with a high iteration limit is bounded by the few waves that hold
        // never-escaping pixels: each runs its millions of steps at the pace of a wave that is alone on its SIMD, and the
        // frame ends that long after the LAST of them was dispatched -- later still where two of them share a SIMD.  A
        // probe launch runs the centre pixel of every 8 x 8 tile for n_iterations / 32 steps (one lane per tile), the
        // tiles whose centre (or a neighbour's) is still running then are launched first -- one per SIMD while there are
        // no more of them than SIMDs -- the rest in their natural order.  Which wave renders which tile changes no pixel.
        const uint32_t tiles_x = (r->width + 7u) / 8u, tiles_y = (r->local_rows + 7u) / 8u;
        const uint32_t n_slots = fsk_tile_launch_waves(A.frame);
        const bool reorder = !use_bla && !r->stats_on && A.frame.wide == 0u && n_iterations >= kTileOrderMinIterations &&
                             n_slots >= kTileOrderMinTiles && (r->variant & FS_VARIANT_FLAG_NATURAL_ORDER) == 0 &&
                             (r->variant & FS_VARIANT_BASE_MASK) == FS_VARIANT_TUNED;
        if (reorder) {
            FS_TRY(buf_reserve(r, r->tile_probe, (size_t)tiles_x * tiles_y * sizeof(uint32_t), kFrame));
            FS_TRY(buf_reserve(r, r->tile_order, ((size_t)n_slots + 1) * sizeof(uint32_t), kFrame, &r->po_order_valid));
        }
        TimedLaunch t(r);
        r->last_frame_ordered = false;
        if (reorder) {
            // the order in r->tile_order is the probe's answer for exactly these inputs: a repeated frame (a viewer redraws a
            // view; every bench step) reuses it and the probe launch is skipped
            const fs_renderer::CostKey key{r->width, r->local_rows, A.frame.band_first, A.frame.band_rows,
                                           A.frame.band_stride, r->orbit_gen};
            const bool warm = r->po_order_valid && r->po_order_key == key && r->po_order_epoch == r->orbit_epoch &&
                              r->po_order_iterations == n_iterations && memcmp(r->po_order_coords, coords, 32) == 0;
            if (!warm) {
                FsBlaArgsT<float> P = A;
                P.probe_out = r->tile_probe.as<uint32_t>();
                P.probe_pitch = tiles_x;
                P.n_iterations = (uint32_t)(n_iterations / kTileProbeDivisor);
                fsk_perturb_scalar_hdr32(P, use_bla, false, r->variant, r->compute);
                fsk_tile_order(P.probe_out, tiles_x, tiles_x, tiles_y, P.n_iterations, r->tile_order.as<uint32_t>(), n_slots,
                               r->compute);
                r->po_order_key = key;
                r->po_order_epoch = r->orbit_epoch;
                r->po_order_iterations = n_iterations;
                memcpy(r->po_order_coords, coords, 32);
                r->po_order_valid = true;
            }
            r->last_frame_ordered = warm;
            A.tile_order = r->tile_order.as<uint32_t>();
        }
        fsk_perturb_scalar_hdr32(A, use_bla, r->stats_on, r->variant, r->compute);
    } else {
        FsBlaArgsT<double> A;
        init_args(r, A, n_iterations);
        A.zref = r->zref64;
        A.levels = (const fs_bla_hdr64 *const *)r->bla_levels_dev;
        A.queue = r->queue;
        fill_coords(A.coords, coords);
        A.orbit_count = (uint32_t)r->orbit_uncompressed;
        A.lm2 = r->bla_lm2;
        TimedLaunch t(r);
        fsk_perturb_scalar_hdr64(A, use_bla, r->stats_on, r->variant, r->compute);
    }
    return (uint32_t)hipGetLastError();
}

uint32_t fs_render_lav2(fs_renderer *r, int type_tag, int mode, int parity, const void *coords, uint64_t n_iterations)
{
    const bool plain = type_tag == FS_T_F32 || type_tag == FS_T_F64 || type_tag == FS_T_2X32;
    const bool hdr = type_tag == FS_T_HDR32 || type_tag == FS_T_HDR64;
    // iteration caps of 2^32 and above need IterType = uint64_t (an 8-byte buffer): every type then runs an instantiation
    // of its kernel that counts in 64 bits (the literal one for HDRFloat<float|double>)
    uint32_t rc;
    const Begin b = render_begin(r, hdr || plain || type_tag == FS_T_HDR2X32, n_iterations, &rc);
    if (b == Begin::kNoFrame)
        return rc;
    r->last_frame_ordered = false; // (every path below that uses a recorded order says so itself)
    r->lav2_last_ordered = false;
    r->last_cold_ordered = false;
    if (b == Begin::kRefused)
        return rc;
    // (the 64-bit counting kernels can also be forced at small caps: FS_VARIANT_WIDE_COUNTERS, a test switch)
    const bool wide = n_iterations > 0xFFFFFFFFull || (r->variant & FS_VARIANT_FLAG_WIDE) != 0;
    if (!r->orbit_ok || r->orbit_type != type_tag)
        return FS_ERR_6; // GPU_Render.cu:1015-1022
    // Perturbation-only with CPU parity: no dispatched CPU RenderAlgorithm is perturbation-only in HDRFloatComplex arithmetic;
    // the parity target is the single-step branch of CalcCpuPerturbationFractalBLA, the scalar kernel
    const bool po_cpu = mode == FS_LAV2_PO && parity == FS_PARITY_CPU;
    const bool no_table = mode != FS_LAV2_PO && (!r->la_ok || r->la_type != type_tag);
    if (r->orbit_seq && hdr) {
        if (po_cpu)
            return FS_ERR_UNSUPPORTED; // the scalar kernel reads an expanded orbit: not served in this mode
        return no_table ? FS_ERR_6 : lav2_seq(r, type_tag, mode, parity, coords, n_iterations, wide);
    }
    if (r->la_u64 && mode != FS_LAV2_PO)
        return FS_ERR_UNSUPPORTED; // the table is in the uint64_t layout: only the waypoint-resident kernel reads it
    if (wide && hdr && !po_cpu)
        return no_table ? FS_ERR_6 : lav2_wide(r, type_tag, mode, parity, coords, n_iterations);
    if (plain)
        return no_table ? FS_ERR_6 : lav2_plain(r, type_tag, mode, coords, n_iterations);
    if (type_tag == FS_T_HDR2X32)
        return no_table ? FS_ERR_6 : lav2_2x32(r, mode, coords, n_iterations);
    if (po_cpu) {
        const int32_t saved = r->bla_n_levels;
        r->bla_n_levels = 0;
        const uint32_t e = fs_render_bla(r, type_tag, coords, n_iterations);
        r->bla_n_levels = saved;
        return e;
    }
    if (no_table)
        return FS_ERR_6;
    return type_tag == FS_T_HDR32 ? lav2_hdr32(r, mode, parity, coords, n_iterations)
                                  : lav2_hdr64(r, mode, parity, coords, n_iterations);
}

uint32_t fs_render_direct(fs_renderer *r, int type_tag, const void *coords, uint64_t n_iterations)
{
    uint32_t rc;
    if (render_begin(r, type_tag == FS_T_F64 || type_tag == FS_T_HDR32 || type_tag == FS_T_HDR64, n_iterations, &rc) != Begin::kGo)
        return rc;
    FS_TRY(buf_reserve(r, r->cx_row, (size_t)16 * r->width, kFrame));
    if (type_tag == FS_T_F64) {
        const double *c = (const double *)coords;
        FsDirectArgs64 A;
        init_args(r, A, n_iterations);
        A.cx_row = r->cx_row.as<double>();
        A.dy = c[1];
        A.maxY = c[3];
        TimedLaunch t(r);
        fsk_direct_f64(A, c[2], c[0], r->stats_on, r->compute);
    } else if (type_tag == FS_T_HDR32) {
        const fs_real_hdr32 *c = (const fs_real_hdr32 *)coords;
        FsDirectHdrArgsT<float> A;
        init_args(r, A, n_iterations);
        A.cx_row = r->cx_row.as<fs::hreal<float>>();
        A.dy = fs::hreal32{c[1].m, c[1].e};
        A.maxY = fs::hreal32{c[3].m, c[3].e};
        TimedLaunch t(r);
        fsk_direct_hdr32(A, fs::hreal32{c[2].m, c[2].e}, fs::hreal32{c[0].m, c[0].e}, r->stats_on, r->compute);
    } else {
        const fs_real_hdr64 *c = (const fs_real_hdr64 *)coords;
        FsDirectHdrArgsT<double> A;
        init_args(r, A, n_iterations);
        A.cx_row = r->cx_row.as<fs::hreal<double>>();
        A.dy = fs::hreal64{c[1].m, c[1].e};
        A.maxY = fs::hreal64{c[3].m, c[3].e};
        TimedLaunch t(r);
        fsk_direct_hdr64(A, fs::hreal64{c[2].m, c[2].e}, fs::hreal64{c[0].m, c[0].e}, r->stats_on, r->compute);
    }
    return (uint32_t)hipGetLastError();
}

uint32_t fs_render_scaled(fs_renderer *r, int type_tag, const void *coords, uint64_t n_iterations)
{
    uint32_t rc;
    if (render_begin(r, type_tag == FS_T_HDR32 || type_tag == FS_T_F64, n_iterations, &rc) != Begin::kGo)
        return rc;
    if (!r->scaled_t || !r->scaled_f || r->scaled_count < 2 || r->scaled_type != type_tag)
        return FS_ERR_6;
    const float w2threshold = (float)exp(log((double)1e30f) / 2.0);
    if (type_tag == FS_T_F64) {
        FsScaledArgsF64 A;
        init_args(r, A, n_iterations);
        A.orbit_t = (const fs_orbit_f64_bad *)r->scaled_t;
        A.orbit_f = r->scaled_f;
        const double *c = (const double *)coords;
        A.dx = c[0], A.dy = c[1], A.centerX = c[2], A.centerY = c[3];
        A.orbit_count = (uint32_t)r->scaled_count;
        A.w2threshold = w2threshold;
        TimedLaunch t(r);
        fsk_scaled_f64(A, r->stats_on, r->variant & FS_VARIANT_BASE_MASK, r->compute);
        return (uint32_t)hipGetLastError();
    }
    FsScaledArgs32 A;
    init_args(r, A, n_iterations);
    A.orbit_t = (const fs_orbit_hdr32_bad *)r->scaled_t;
    A.orbit_f = r->scaled_f;
    fill_coords(A.coords, coords);
    A.orbit_count = (uint32_t)r->scaled_count;
    A.w2threshold = w2threshold;
    TimedLaunch t(r);
    fsk_scaled_hdr32(A, r->stats_on, r->variant & FS_VARIANT_BASE_MASK, r->compute);
    return (uint32_t)hipGetLastError();
}

uint32_t fs_render_direct_lp(fs_renderer *r, int type_tag, const void *coords, uint64_t n_iterations,
                             int iteration_precision)
{
    uint32_t rc;
    if (render_begin(r, type_tag == FS_T_F32 || type_tag == FS_T_2X32 || type_tag == FS_T_2X64 || type_tag == FS_T_4X32 ||
                            type_tag == FS_T_4X64, n_iterations, &rc) != Begin::kGo)
        return rc;
    FsDirectLpArgs A;
    init_args(r, A, n_iterations);
    if (type_tag == FS_T_F32)
        memcpy(A.c32, coords, 4 * sizeof(float));
    else if (type_tag == FS_T_2X32)
        memcpy(A.c32, coords, 8 * sizeof(float));
    else if (type_tag == FS_T_4X32)
        memcpy(A.c32, coords, 16 * sizeof(float));
    else if (type_tag == FS_T_4X64)
        memcpy(A.c64, coords, 16 * sizeof(double));
    else
        memcpy(A.c64, coords, 8 * sizeof(double));
    const int kind = type_tag == FS_T_F32    ? 0
                     : type_tag == FS_T_2X32 ? 1
                     : type_tag == FS_T_2X64 ? 2
                     : type_tag == FS_T_4X32 ? 3
                                             : 4;
    TimedLaunch t(r);
    (void)fsk_direct_lp(A, kind, iteration_precision, r->stats_on, r->compute);
    return (uint32_t)hipGetLastError();
}

uint32_t fs_set_kernel_variant(fs_renderer *r, int variant)
{
    const int base = variant & FS_VARIANT_BASE_MASK, flags = variant & ~FS_VARIANT_BASE_MASK;
    if (base > FS_VARIANT_TUNED_NOSCALE ||
        (flags & ~(FS_VARIANT_FLAG_LDS_ORBIT | FS_VARIANT_FLAG_REFILL | FS_VARIANT_FLAG_WIDE | FS_VARIANT_FLAG_NATURAL_ORDER |
                   FS_VARIANT_FLAG_BLA_POOL)) != 0)
        return hipErrorInvalidValue;
    r->variant = base | flags;
    return 0;
}

uint32_t fs_forget_tile_costs(fs_renderer *r)
{
    r->lav2_cost_valid = false;
    r->po_order_valid = false;
    r->pix_valid = false;
    r->pix_seen = false;
    r->at_order_valid = false;
    return 0;
}

int fs_last_frame_tile_ordered(fs_renderer *r) { return r->last_frame_ordered ? 1 : 0; }
int fs_last_frame_sampled_tile_order(fs_renderer *r) { return r->last_cold_ordered ? 1 : 0; }

uint32_t fs_read_tile_costs(fs_renderer *r, uint32_t *out, uint64_t max_words, uint64_t *n_tiles)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->lav2_cost.p || !r->lav2_cost_valid)
        return FS_ERR_6;
    const uint64_t n = (uint64_t)((r->lav2_cost_key.width + 7u) / 8u) * ((r->lav2_cost_key.local_rows + 7u) / 8u);
    if (n_tiles)
        *n_tiles = n;
    const uint64_t m = n < max_words ? n : max_words;
    if (out && m) {
        FS_TRY(hipMemcpyAsync(out, r->lav2_cost.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, r->compute));
        FS_TRY(hipStreamSynchronize(r->compute));
    }
    return 0;
}

uint32_t fs_seq_cursor_probe(fs_renderer *r, int wide_positions, uint64_t start, uint32_t n, void *out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->orbit_ok || !r->orbit_seq || !r->wp_raw || !out)
        return FS_ERR_6;
    const bool is64 = r->orbit_type == FS_T_HDR64;
    const size_t rec = is64 ? sizeof(fs::hcplx<double>) : sizeof(fs::hcplx<float>);
    void *dev = nullptr;
    FS_TRY(r_alloc(r, &dev, (size_t)n * rec, kFrame));
    fsk_seq_cursor_probe(is64, wide_positions != 0, r->wp_raw, (uint32_t)r->orbit_size,
                         is64 ? (const void *)&r->c_low64[0] : (const void *)&r->c_low32[0],
                         is64 ? (const void *)&r->c_low64[1] : (const void *)&r->c_low32[1], start, n, dev, r->compute);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess)
        err = hipMemcpyAsync(out, dev, (size_t)n * rec, hipMemcpyDeviceToHost, r->compute);
    if (err == hipSuccess)
        err = hipStreamSynchronize(r->compute);
    (void)r_free(r, dev);
    return (uint32_t)err;
}

uint32_t fs_read_tile_order(fs_renderer *r, uint32_t *out, uint64_t max_words)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->lav2_order.p || !r->lav2_last_ordered)
        return FS_ERR_6;
    const uint64_t n = (uint64_t)((r->lav2_cost_key.width + 7u) / 8u) * ((r->lav2_cost_key.local_rows + 7u) / 8u);
    const uint64_t m = n < max_words ? n : max_words;
    FS_TRY(hipMemcpyAsync(out, r->lav2_order.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, r->compute));
    FS_TRY(hipStreamSynchronize(r->compute));
    return 0;
}

uint32_t fs_enable_step_count(fs_renderer *r, int enable)
{
    r->stats_on = enable != 0;
    return 0;
}

static uint32_t test_threshold(fs_renderer *r, const int32_t *bound_bits, const int32_t *scale_shift, const int32_t *dc_bits,
                               int32_t *threshold_out, uint32_t n, bool ndz);

uint32_t fs_test_block_threshold(fs_renderer *r, const int32_t *bound_bits, const int32_t *scale_shift, const int32_t *dc_bits,
                                 int32_t *threshold_out, uint32_t n)
{
    return test_threshold(r, bound_bits, scale_shift, dc_bits, threshold_out, n, false);
}

uint32_t fs_test_ndz_threshold(fs_renderer *r, const int32_t *bound_bits, const int32_t *scale_shift, const int32_t *dc_bits,
                               int32_t *threshold_out, uint32_t n)
{
    return test_threshold(r, bound_bits, scale_shift, dc_bits, threshold_out, n, true);
}

static uint32_t test_threshold(fs_renderer *r, const int32_t *bound_bits, const int32_t *scale_shift, const int32_t *dc_bits,
                               int32_t *threshold_out, uint32_t n, bool ndz)
{
    if (!r || !bound_bits || !scale_shift || !dc_bits || !threshold_out)
        return (uint32_t)hipErrorInvalidValue;
    if (n == 0)
        return 0;
    FS_TRY(hipSetDevice(r->device));
    int *d = nullptr;
    FS_TRY(hipMalloc((void **)&d, (size_t)n * 4 * sizeof(int)));
    uint32_t rc = (uint32_t)hipMemcpy(d, bound_bits, n * sizeof(int), hipMemcpyHostToDevice);
    if (!rc)
        rc = (uint32_t)hipMemcpy(d + n, scale_shift, n * sizeof(int), hipMemcpyHostToDevice);
    if (!rc)
        rc = (uint32_t)hipMemcpy(d + 2 * (size_t)n, dc_bits, n * sizeof(int), hipMemcpyHostToDevice);
    if (!rc) {
        if (ndz)
            fsk_test_ndz_threshold(d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n, n, r->compute);
        else
            fsk_test_block_threshold(d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n, n, r->compute);
        rc = (uint32_t)hipGetLastError();
    }
    if (!rc)
        rc = (uint32_t)hipStreamSynchronize(r->compute);
    if (!rc)
        rc = (uint32_t)hipMemcpy(threshold_out, d + 3 * (size_t)n, n * sizeof(int), hipMemcpyDeviceToHost);
    hipFree(d);
    return rc;
}

uint32_t fs_read_stats_raw(fs_renderer *r, uint64_t *out, uint64_t max_words)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->stats)
        return FS_ERR_6;
    const size_t n = r->stats_words < max_words ? r->stats_words : (size_t)max_words;
    FS_TRY(hipMemcpyAsync(out, r->stats, n * sizeof(uint64_t), hipMemcpyDeviceToHost, r->compute));
    FS_TRY(hipStreamSynchronize(r->compute));
    return 0;
}

uint32_t fs_read_step_count(fs_renderer *r, uint64_t counts[8])
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->stats)
        return FS_ERR_6;
    // the 64-bit counting instantiations are not built with the step counters: zeros would read as "no work was done"
    if (r->last_launch_wide)
        return FS_ERR_UNSUPPORTED;
    // ordered behind the kernels of the (non-blocking) compute stream, which the null stream is not
    FS_TRY(hipMemcpyAsync(counts, r->stats, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, r->compute));
    FS_TRY(hipStreamSynchronize(r->compute));
    return 0;
}

} // extern "C"
