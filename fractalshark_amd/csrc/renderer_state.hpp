// renderer_state.hpp -- what the host translation units of libfsmi355.so (renderer*.cpp) share: the state of one renderer and the
// helpers that more than one of them calls (namespace fsr).  Host only: no kernel translation unit includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "../../include/fsmi355_internal.h"
#include "kernels.h"

#define FS_TRY(expr)                                                                                                  \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess)                                                                                         \
            return (uint32_t)e_;                                                                                      \
    } while (0)

// A device buffer that only grows: the pointer and the bytes behind it in one place, so that neither outlives the other
// (buf_reserve / buf_release below, on top of r_alloc / r_free).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0; // bytes
    template <class T> T *as() const { return (T *)p; }
};

struct ExactLayout; // (renderer_exact.cpp) the device block of one exact call

struct fs_renderer {
    int device = 0;
    hipStream_t compute = nullptr;
    hipStream_t display = nullptr;
    // HIP events around the iteration-kernel launches, a ring of pairs: fs_last_kernel_ms reads the newest one,
    // fs_kernel_ms_history the last few (frames that are in flight together, e.g. a pipelined bench loop, each keep theirs)
    static constexpr uint32_t kTimingRing = 64;
    hipEvent_t ev_start[kTimingRing] = {}, ev_stop[kTimingRing] = {};
    // a frame made of two kernels (HDRFloat<double> LAv2: the AT pass, then the frame's kernel) also records where the first one
    // ended (fs_kernel_ms_split_history); created on first use
    hipEvent_t ev_mid[kTimingRing] = {};
    bool mid_valid[kTimingRing] = {};
    uint64_t timed_launches = 0; // launches recorded so far; launch i uses pair i % kTimingRing

    // geometry
    uint32_t width = 0, height = 0, aa = 0, iter_bytes = 0;
    uint32_t w_block = 0, h_block = 0;
    uint32_t color_w = 0, color_h = 0;
    size_t n_cu = 0, n_color_cu = 0;
    uint32_t band_first = 0, band_rows = 0, band_stride = 0; // 0 rows = whole frame
    uint32_t local_rows = 0, local_rows_padded = 0;

    // buffers
    DevBuf iters_internal;
    void *iters_external = nullptr;
    size_t iters_external_bytes = 0;
    fs_reduction reduce_seed{}; // source of the stream-ordered seed copy in fs_render_current (must outlive the call)
    fs_color16 *colors = nullptr;
    fs_reduction *reduction = nullptr;
    uint64_t *stats = nullptr;
    size_t stats_words = 40;

    uint32_t *queue = nullptr; // pixel counter of the persistent launches (kernels_perturb.hip, k_perturb_scalar)
    DevBuf tile_probe, tile_order; // "long tiles first" (fs_render_bla): probe counts, launch order (uint32_t each)
    // "longest tiles first" of the tuned LAv2 kernel (fs_render_lav2): the costs the last frame recorded per 8 x 8 tile, the
    // launch order made from them, work memory of the sort; and what the costs belong to (a frame of another geometry, band
    // layout or orbit generation starts cold: natural order, costs recorded)
    DevBuf lav2_cost, lav2_order, lav2_sort_tmp; // (uint32_t each)
    bool lav2_cost_valid = false;
    struct CostKey {
        uint32_t width, local_rows, band_first, band_rows, band_stride;
        uint64_t orbit_gen;
        bool operator==(const CostKey &o) const
        {
            return width == o.width && local_rows == o.local_rows && band_first == o.band_first && band_rows == o.band_rows &&
                   band_stride == o.band_stride && orbit_gen == o.orbit_gen;
        }
    } lav2_cost_key{};
    // fs_render_bla's probe order is a pure function of (geometry, bands, orbit, coordinates, iteration limit): the next frame
    // with the same inputs reuses it and skips the probe launch (round 4; ~9 ms of C2's frame)
    bool po_order_valid = false;
    CostKey po_order_key{};
    uint64_t po_order_epoch = 0, po_order_iterations = 0;
    unsigned char po_order_coords[32] = {};
    bool last_frame_ordered = false; // the last fs_render_lav2 launch used a recorded order (fs_last_frame_tile_ordered)
    // "pixels in the order of the previous frame's counts" (kernels_order.hip; HDRFloat<double> and HDRFloat<CudaDblflt> LAv2):
    // the order, the sort's work memory, and what the order was made from
    // HDRFloat<double> LAv2: PerformAT in a pass of its own (fsk_at_pass64) with its own pixel order -- its results, the AT
    // iterations every pixel needs by itself (recorded by the first frame of a view), and the order made from them
    DevBuf at_res, at_cost, at_order; // FsAtRes[], uint32_t[], uint32_t[]
    bool at_order_valid = false; // ... for at_key (set where at_order is built: the order is a permutation of THAT key's buffer)
    DevBuf pix_cost; // per-pixel cost the unordered frame of a view records; what the order is sorted by
    DevBuf pix_order, pix_work, pix_temp;
    bool pix_valid = false;
    bool pix_seen = false; // the last unordered frame's key (pix_seen_key): an order is only made for a view that comes twice
    struct PixKey {
        uint32_t rounded_width, local_rows, band_first, band_rows, band_stride;
        int type_tag, mode, parity;
        uint64_t orbit_gen, orbit_epoch, n_iterations;
        unsigned char coords[64];
        bool operator==(const PixKey &o) const { return memcmp(this, &o, sizeof(*this)) == 0; }
    } pix_key{}, pix_seen_key{}, at_key{};
    // (round 6) an order for a view's FIRST frame: tiles by a sampled PerformAT count (kernels_tile_sample.hip)
    DevBuf cold_cost, cold_order, cold_work, cold_temp;
    bool last_cold_ordered = false; // (fs_last_frame_sampled_tile_order)
    bool lav2_last_ordered = false; // the last launch was an HDRFloat<float> frame in its recorded TILE order (fs_read_tile_order)
    bool last_launch_wide = false;   // the last render launched a 64-bit counting kernel: those carry no step counters
    bool stats_on = false;
    int variant = FS_VARIANT_TUNED;

    // palette (GPU_Render.cu:270-304)
    fs_color16 *pal = nullptr;
    uint32_t pal_iters = 0, pal_aux_depth = 0;
    const fs_color16 *pal_cached_host = nullptr;
    uint64_t pal_cached_gen = 0;

    // orbit (HDRFloat<float>)
    uint64_t orbit_gen = 0;
    // counts orbit uploads whose content differs from the one before (a generation of 0 means "not cached": it does not
    // identify an orbit, and RenderPerturbBLA re-uploads the same orbit on every call as the reference does -- a sampled
    // fingerprint of the entries tells a repeated upload from a new orbit; it only decides whether a recorded tile order
    // is reused, never a pixel)
    uint64_t orbit_epoch = 0, orbit_fp = 0, pending_fp = 0;
    bool orbit_ok = false;
    int orbit_type = -1; // FS_T_HDR32 / FS_T_HDR64 / FS_T_HDR2X32 / FS_T_F64
    fs_orbit_2x32 *orbit_2x32 = nullptr; // HDRFloat<CudaDblflt> orbit (FS_T_HDR2X32), used as uploaded
    int scaled_type = -1;
    void *scaled_t = nullptr; // PerturbExtras::Bad orbits of the scaled kernel (fs_orbit_hdr32_bad[] or fs_orbit_f64_bad[])
    fs_orbit_f32_bad *scaled_f = nullptr;
    uint64_t scaled_count = 0;
    float4 *zref = nullptr;
    float4 *zq = nullptr; // companions of zref for the tuned LAv2 loop (2 x zq_n entries)
    uint64_t zq_n = 0;
    float2 *zs2 = nullptr; // (inside the zq block) compact companions of the 16-step body
    float4 *zqb = nullptr;
    float2 *znz = nullptr; // (inside the zq block) NDZ body bounds of the tuned LAv2 loop
    FsZ64 *zref64 = nullptr;
    fs_orbit_f64 *orbit_f64 = nullptr; // plain double orbit (FS_T_F64), used as uploaded
    void *orbit_plain = nullptr;       // plain float / CudaDblflt orbit (FS_T_F32 / FS_T_2X32), used as uploaded
    alignas(8) uint8_t at_plain[sizeof(fs_at_f64_u32)] = {0}; // ATInfo of the plain LA table (type = la_type)
    uint64_t orbit_size = 0, orbit_uncompressed = 0, orbit_period = 0;
    // PerturbExtras::SimpleCompression orbits: 0 = expanded once on upload (default), 1 = kept compressed, decompressed by
    // the kernel as it walks the orbit (fs_set_compressed_orbit_mode)
    int compressed_mode = 0;
    bool orbit_seq = false; // the resident orbit is a compressed one (wp_raw); zref / zref64 are NULL
    void *wp_raw = nullptr; // fs_orbit_hdr32_rc[] / fs_orbit_hdr64_rc[]
    fs_real_hdr32 c_low32[2] = {};
    fs_real_hdr64 c_low64[2] = {};
    alignas(8) uint8_t c_low_plain[2][16] = {}; // ... of a float / double / CudaDblflt / HDRFloat<CudaDblflt> orbit (as uploaded)

    // LA table
    uint64_t la_gen = 0;
    bool la_ok = false;
    int la_type = -1;
    DevBuf las;    // fs_la_hdr32_u32[] or fs_la_hdr64_u32[]; reused by the next table when it fits
    DevBuf stages; // fs_la_stage_u32[]
    uint32_t n_las = 0, n_stages = 0;
    int la_valid = 0, use_at = 0;
    bool la_u64 = false;     // `las` holds the reference's uint64_t records (only the waypoint-resident wide kernel reads them)
    uint32_t at_step_hi = 0; // high word of the AT step length of a uint64_t table
    fs_at_hdr32_u32 at{};
    fs_at_hdr64_u32 at64{};
    fs_at_2x32_u32 at2x32{};

    // BLA table
    std::vector<void *> bla_level_mem;
    std::vector<uint64_t> bla_level_sizes;
    const void **bla_levels_dev = nullptr;
    int bla_type = -1;
    int32_t bla_n_levels = 0, bla_lm2 = 0;

    // direct kernels
    DevBuf cx_row; // double[] / hreal<float>[] / hreal<double>[] (16 B per column is enough for all)

    // memory management (r_alloc / r_free below)
    std::vector<void *> host_allocs; // input tables that live in page-locked HOST memory (device out of memory)
    // device blocks of this renderer (synchronous allocation): every live block with its size, and the released ones that
    // are kept for the next request of a similar size (r_alloc / r_free)
    struct Block {
        void *p;
        size_t bytes;
    };
    std::vector<Block> live_blocks, kept_blocks;
    std::mutex kept_mu; // kept_blocks only: another renderer of the same device may drain them when IT runs out of memory
    size_t host_alloc_bytes = 0;
    uint32_t feature_slice = 0;      // fs_set_feature_slice (tests): steps per launch of the Feature Finder evaluators, 0 = default
    // The exact renderer's kept set: ONE live device block (no idle memory: r_alloc's, never r_free'd while it is valid) with one
    // list -- [head | cx | cy | the parked samples | proved plane], the ExactLayout that layout() returns -- and what the call was
    // given.  It describes the frame in the iteration buffer: whatever writes, clears or replaces that buffer drops it
    // (fsr::exact_drop_kept).
    struct ExactKept {
        char *blk = nullptr;
        bool valid = false, wide = false, cycle = false;
        uint32_t samples = 0, W = 0, H = 0;
        uint64_t proved = 0, cap = 0;
        uint32_t frac_bits = 0, limbs = 0, bailout = 0;
        int inclusive = 0;
        ExactLayout layout() const; // (renderer_exact.cpp) the one place that says how blk is laid out
    };
    // What the exact renderers keep between calls; renderer_exact.cpp alone reads and writes it.
    struct Exact {
        uint32_t slice = 0;          // fs_set_exact_slice (tests, tools): steps per lane per launch of the exact renderer, 0 = default
        bool no_compaction = false;  // ... and its A/B switch: every sample keeps its slot from slice to slice
        uint64_t stats[4] = {};      // fs_read_exact_stats: what the last exact frame did
        bool cycle_check = false;    // fs_set_exact_cycle_check: the lane-per-sample kernels prove non-escape by a repeat of the state
        uint32_t cycle_fp_bits = 0;  // fs_set_exact_cycle_fingerprint_bits (tests): low bits the fingerprint keeps, 0 = all 64
        uint64_t cycle_stats[2] = {}; // fs_read_exact_cycle_stats: samples finished by proof, checkpoints read back
        std::vector<uint8_t> proved; // fs_read_exact_proved: the proved mask of the last fs_render_exact / fs_exact_audit ...
        bool proved_valid = false;   // ... when the last exact call ran with the check on
        bool keep = false;           // fs_set_exact_keep: the two exact renderers leave a kept set for fs_render_exact_continue
        ExactKept kept;
        bool periods = false;        // fs_set_exact_periods: fs_render_exact leaves the period planes (read by no other entry point)
        uint32_t atom_key_bits = 0;  // fs_set_exact_atom_key_bits (tests): top bits the minimum's key keeps, 0 = all 64
        std::vector<uint64_t> atom, cyclen; // fs_read_exact_atom_periods, fs_read_exact_cycle_lengths: the planes of the last ...
        bool atom_valid = false, cyclen_valid = false; // ... fs_render_exact, when it ran with the switch (and the cycle check) on
        // What every exact entry point does to the statistics before it starts.  keep_proved: the call leaves the mask of
        // fs_read_exact_proved as it is (the shifted frames of fs_exact_stable_mask with the check on).
        void reset_stats(bool keep_proved = false)
        {
            memset(stats, 0, sizeof stats);
            memset(cycle_stats, 0, sizeof cycle_stats);
            if (!keep_proved)
                proved_valid = false;
        }
    } exact;
    uint32_t az_gather_rows = 0;     // fs_set_autozoom_gather_cap (tests): frame rows the FilamentTip gather buffer holds, 0 = default
    FsAzStats az_seed{};             // source of the stream-ordered seed copy in fs_autozoom_pick (must outlive the copy)
    bool inject_input_oom = false;   // fault injection: FSMI355_FAIL_INPUT_ALLOC=1 at fs_create time
    DevBuf arena;                    // work memory of fs_build_la (kept between calls, grown on demand)
    uint32_t *la_mail = nullptr;     // 32 words of coherent page-locked memory the build's kernels report through (k_la_mail)
    uint32_t la_mail_seq = 0;
    DevBuf bla_block;                // ONE allocation for the BLA table: the level pointer table, then the levels
    // device-native form of an HDRFloat<float> BLA table (FsBlaRec + ladder, kernels.h): [flag word | records | ladder]
    DevBuf bla_native;
    bool bla_native_ok = false;
    bool bla_native_stale = false; // table or orbit changed since the native form was made: remade by the next BLA render
    uint32_t bla_native_total = 0;
    // the heap-numbered copy the hand-written kernel reads (kernels_bla_fast.hip), made with the native form
    DevBuf bla_heap;
    bool bla_heap_ok = false;
    uint64_t bla_heap_positions = 0;
    uint32_t bla_heap_nq = 0;
    uint32_t bla_level_off[kBlaMaxLevels] = {0};

    void *iters() const { return iters_external ? iters_external : iters_internal.p; }
    bool memory_initialized() const { return iters() != nullptr && width != 0; }
};

namespace fsr {

uint32_t use_device(const fs_renderer *r);

// The renderer's two streams and its timing events, made once: by fs_init_memory, or by fs_feature_eval_direct on a renderer that
// has no frame yet.
uint32_t ensure_streams(fs_renderer *r);

// ---- Device memory of a renderer.
// hipMalloc / hipFree behind a synchronisation of the compute stream (everything that touches such memory is enqueued on
// the compute stream or behind a synchronisation of it); optionally stream-ordered (hipMallocAsync / hipFreeAsync, as the
// reference does, GPU_Render.cu:127,142-153,362-395) -- see async_alloc_enabled() for why that is not the default.
// kInput allocations -- reference orbit, LA table, BLA table, their upload staging -- fall back to page-locked HOST memory
// when the device allocation fails, and the kernels then read them over the bus: slow, but the frame still renders
// (GPUPerturbSingleResults, Perturb.cuh:51-61; GPU_LAReference, GPU_LAReference.h:93-113).  Frame buffers (kFrame) do not.
enum AllocKind { kFrame = 0, kInput = 1 };

hipError_t r_alloc(fs_renderer *r, void **out, size_t bytes, AllocKind kind);
template <class T> hipError_t r_alloc(fs_renderer *r, T **out, size_t bytes, AllocKind kind)
{
    return r_alloc(r, (void **)out, bytes, kind);
}

hipError_t r_free(fs_renderer *r, const void *cp);

// Frees a block and forgets it in the same breath.
template <class T> hipError_t r_release(fs_renderer *r, T *&p)
{
    const hipError_t e = r_free(r, p);
    p = nullptr;
    return e;
}

void buf_release(fs_renderer *r, DevBuf &b);

// At least `bytes` behind every buffer of a group that lives and dies together (the sort's order / work / temp, ...).  When
// one of them is too small ALL are freed, then allocated again in the order given; a failed allocation leaves the whole
// group released and is returned -- whether that is an error or "run without it" is the caller's decision (the sticky
// error is still the caller's to clear).  *valid, when given, describes contents that index the group (a recorded order):
// it is cleared whenever the buffers are replaced.
struct BufWant {
    DevBuf *buf;
    size_t bytes;
};
hipError_t buf_reserve(fs_renderer *r, std::initializer_list<BufWant> group, AllocKind kind, bool *valid = nullptr);
hipError_t buf_reserve(fs_renderer *r, DevBuf &b, size_t bytes, AllocKind kind, bool *valid = nullptr);

hipError_t la_reserve(fs_renderer *r, size_t las_bytes, size_t stages_bytes); // (renderer_inputs.cpp)

// The orbit, the LA table and the BLA table go (fs_init_memory with a new geometry, fs_destroy).
void free_perturb(fs_renderer *r);
uint32_t bla_make_native(fs_renderer *r, int32_t n_levels); // (renderer_inputs.cpp)
// The exact renderer's kept set goes (renderer_exact.cpp): called by whatever writes, clears or replaces the iteration buffer.
// Nothing kept: nothing happens, not even a synchronisation.
void exact_drop_kept(fs_renderer *r);

struct TimedLaunch {
    fs_renderer *r;
    explicit TimedLaunch(fs_renderer *rr) : r(rr)
    {
        if (r->ev_start[0]) {
            hipEventRecord(r->ev_start[r->timed_launches % fs_renderer::kTimingRing], r->compute);
            r->mid_valid[r->timed_launches % fs_renderer::kTimingRing] = false;
        }
        if (r->stats_on && r->stats)
            hipMemsetAsync(r->stats, 0, (r->stats_words == 40 ? 40 : 8) * sizeof(uint64_t), r->compute);
    }
    void mid() // between the two kernels of a two-kernel frame
    {
        if (!r->ev_start[0])
            return;
        const uint32_t i = (uint32_t)(r->timed_launches % fs_renderer::kTimingRing);
        if (!r->ev_mid[i] && hipEventCreate(&r->ev_mid[i]) != hipSuccess) {
            (void)hipGetLastError();
            r->ev_mid[i] = nullptr;
            return;
        }
        if (hipEventRecord(r->ev_mid[i], r->compute) == hipSuccess)
            r->mid_valid[i] = true;
    }
    ~TimedLaunch()
    {
        if (r->ev_stop[0]) {
            hipEventRecord(r->ev_stop[r->timed_launches % fs_renderer::kTimingRing], r->compute);
            r->timed_launches++;
        }
    }
};

} // namespace fsr
