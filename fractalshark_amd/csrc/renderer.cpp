// renderer.cpp -- host side of libfsmi355.so: the C ABI of include/fsmi355.h.
//
// State machine of one reference GPURenderer (FractalSharkGpuLib/GPU_Render.cu:92-1823) re-expressed for
// HIP: two non-blocking streams (compute = lowest priority, display = highest, GPU_Render.cu:247-267),
// device buffers owned here, uploads cached by generation number (GPU_Render.cu:440-487), kernels launched
// asynchronously on the compute stream.  There is NO CPU fallback: if no HIP device is usable every entry
// point returns the HIP error.
//
// This file: create / destroy, device memory, geometry, streams and timing.  The rest of the C ABI by concern:
// renderer_inputs.cpp (orbit, LA and BLA tables), renderer_la_build.cpp (fs_build_la), renderer_launch.cpp (fs_render_*),
// renderer_current.cpp (colouring and read-back), renderer_exact.cpp, renderer_analysis.cpp (Feature Finder, autozoom).
#include "renderer_state.hpp"

#include <algorithm>
#include <cstdlib>
#include <new>

using namespace fsr;

// The stream-ordered allocator (round 3: hipMallocAsync / hipFreeAsync on the compute stream) is OFF by default: on this
// ROCm (7.2.0) a block that the pool hands out again is not reliably the memory the next copy and the next kernel agree on
// -- tools/microbench/async_alloc_probe.hip (upload, transform, check, free, four rounds) finds stale or zero data from
// the second round on with blocks of 32 MiB and more, whatever the release threshold, the stream type or the kind of host
// memory, and none with hipMalloc / hipFree (profiles/r03zz_async_alloc_probe.txt).  In this library it showed as wrong
// frames from the SECOND orbit upload of a renderer when the orbit has tens of millions of entries (Views 10, 15, 22).
// FSMI355_ASYNC_ALLOC=1 switches the stream-ordered path back on.  What keeps allocation off the frame path either way:
// buffers are kept and reused when the next table fits (LA table, BLA table block, work arena, iteration buffers).
static bool async_alloc_enabled()
{
    static const bool on = [] {
        const char *e = getenv("FSMI355_ASYNC_ALLOC");
        return e != nullptr && atoi(e) != 0;
    }();
    return on;
}

constexpr size_t kKeptBlocks = 16;
constexpr size_t kKeptBytes = (size_t)2 << 30;

static uint64_t release_kept_blocks(fs_renderer *r)
{
    std::lock_guard<std::mutex> g(r->kept_mu);
    uint64_t bytes = 0;
    for (const auto &k : r->kept_blocks) {
        (void)hipFree(k.p);
        bytes += k.bytes;
    }
    r->kept_blocks.clear();
    return bytes;
}

// Every renderer of the process, so that one that runs out of device memory can take back what the OTHERS of its device keep
// idle (FractalShark holds four GPURenderers on one device; a kept block is idle by construction -- its owner parked it
// after draining its stream -- so any thread may free it).
static std::mutex g_renderers_mu;
static std::vector<fs_renderer *> g_renderers;

static uint64_t release_idle_memory_of_device(int device)
{
    std::lock_guard<std::mutex> g(g_renderers_mu);
    uint64_t bytes = 0;
    for (fs_renderer *o : g_renderers)
        if (o->device == device)
            bytes += release_kept_blocks(o);
    return bytes;
}

namespace fsr {

uint32_t use_device(const fs_renderer *r)
{
    FS_TRY(hipSetDevice(r->device));
    return 0;
}

hipError_t r_alloc(fs_renderer *r, void **out, size_t bytes, AllocKind kind)
{
    if (bytes == 0)
        bytes = 16;
    *out = nullptr;
    hipError_t e = hipErrorOutOfMemory;
    if (!(kind == kInput && r->inject_input_oom)) {
        if (r->compute && async_alloc_enabled()) {
            e = hipMallocAsync(out, bytes, r->compute);
        } else {
            // a kept block that fits (best fit, at most twice the size asked for) before a new allocation: a host that uploads
            // an orbit and its tables for every frame allocates nothing in the steady state
            {
                std::lock_guard<std::mutex> g(r->kept_mu);
                size_t best = r->kept_blocks.size();
                for (size_t i = 0; i < r->kept_blocks.size(); i++) {
                    const size_t b = r->kept_blocks[i].bytes;
                    if (b >= bytes && b <= 2 * bytes + (1u << 16) &&
                        (best == r->kept_blocks.size() || b < r->kept_blocks[best].bytes))
                        best = i;
                }
                if (best != r->kept_blocks.size()) {
                    *out = r->kept_blocks[best].p;
                    r->live_blocks.push_back(r->kept_blocks[best]);
                    r->kept_blocks.erase(r->kept_blocks.begin() + (long)best);
                    return hipSuccess;
                }
            }
            e = hipMalloc(out, bytes);
            if (e != hipSuccess) { // idle blocks may be what is in the way: this renderer's, then every renderer's of the device
                (void)hipGetLastError();
                if (release_kept_blocks(r) != 0u)
                    e = hipMalloc(out, bytes);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    if (release_idle_memory_of_device(r->device) != 0u)
                        e = hipMalloc(out, bytes);
                }
            }
            if (e == hipSuccess)
                r->live_blocks.push_back(fs_renderer::Block{*out, bytes});
        }
    }
    if (e == hipSuccess || kind != kInput)
        return e;
    (void)hipGetLastError(); // the failed device allocation is handled here, not reported by a later launch check
    e = hipHostMalloc(out, bytes, hipHostMallocDefault); // mapped into the device's address space at the same address
    if (e == hipSuccess) {
        r->host_allocs.push_back(*out);
        r->host_alloc_bytes += bytes;
    }
    return e;
}

hipError_t r_free(fs_renderer *r, const void *cp)
{
    void *p = const_cast<void *>(cp);
    if (!p)
        return hipSuccess;
    for (size_t i = 0; i < r->host_allocs.size(); i++)
        if (r->host_allocs[i] == p) {
            r->host_allocs.erase(r->host_allocs.begin() + (long)i);
            if (r->compute)
                (void)hipStreamSynchronize(r->compute); // a kernel may still be reading it
            return hipHostFree(p);
        }
    if (r->compute && async_alloc_enabled())
        return hipFreeAsync(p, r->compute);
    if (r->compute)
        (void)hipStreamSynchronize(r->compute); // work that uses the block has been enqueued on this stream only
    for (size_t i = 0; i < r->live_blocks.size(); i++)
        if (r->live_blocks[i].p == p) {
            const fs_renderer::Block b = r->live_blocks[i];
            r->live_blocks.erase(r->live_blocks.begin() + (long)i);
            // kept for the next request -- up to kKeptBlocks of them and kKeptBytes in total (the oldest go first)
            std::lock_guard<std::mutex> g(r->kept_mu);
            r->kept_blocks.push_back(b);
            size_t total = 0;
            for (const auto &k : r->kept_blocks)
                total += k.bytes;
            while (!r->kept_blocks.empty() && (r->kept_blocks.size() > kKeptBlocks || total > kKeptBytes)) {
                total -= r->kept_blocks.front().bytes;
                (void)hipFree(r->kept_blocks.front().p);
                r->kept_blocks.erase(r->kept_blocks.begin());
            }
            return hipSuccess;
        }
    return hipFree(p); // (not one of ours: allocated before the compute stream existed, or by the stream-ordered path)
}

void buf_release(fs_renderer *r, DevBuf &b)
{
    (void)r_free(r, b.p);
    b = DevBuf{};
}

hipError_t buf_reserve(fs_renderer *r, std::initializer_list<BufWant> group, AllocKind kind, bool *valid)
{
    bool fits = true;
    for (const BufWant &w : group)
        fits = fits && w.buf->p && w.buf->cap >= w.bytes;
    if (fits)
        return hipSuccess;
    if (valid)
        *valid = false;
    for (const BufWant &w : group)
        buf_release(r, *w.buf);
    for (const BufWant &w : group) {
        const hipError_t e = r_alloc(r, &w.buf->p, w.bytes, kind);
        if (e != hipSuccess) {
            w.buf->p = nullptr;
            for (const BufWant &u : group)
                buf_release(r, *u.buf);
            return e;
        }
        w.buf->cap = w.bytes ? w.bytes : 16; // (what r_alloc hands out for a request of zero)
    }
    return hipSuccess;
}
hipError_t buf_reserve(fs_renderer *r, DevBuf &b, size_t bytes, AllocKind kind, bool *valid)
{
    return buf_reserve(r, {BufWant{&b, bytes}}, kind, valid);
}

uint32_t ensure_streams(fs_renderer *r)
{
    if (r->compute)
        return 0;
    int lo = 0, hi = 0;
    FS_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    FS_TRY(hipStreamCreateWithPriority(&r->compute, hipStreamNonBlocking, lo));
    FS_TRY(hipStreamCreateWithPriority(&r->display, hipStreamNonBlocking, hi));
    for (uint32_t i = 0; i < fs_renderer::kTimingRing; i++) {
        FS_TRY(hipEventCreate(&r->ev_start[i]));
        FS_TRY(hipEventCreate(&r->ev_stop[i]));
    }
    // the stream-ordered allocator keeps freed memory for the next allocation instead of returning it to the driver at
    // every synchronisation (uploads synchronise: their host buffers are borrowed for the call only)
    hipMemPool_t pool = nullptr;
    if (hipDeviceGetDefaultMemPool(&pool, r->device) == hipSuccess && pool) {
        uint64_t keep = ~0ull;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    (void)hipGetLastError();
    return 0;
}

} // namespace fsr

namespace {

void compute_local_rows(fs_renderer *r)
{
    if (r->band_rows == 0 || r->band_rows >= r->height) {
        r->band_first = 0;
        r->band_rows = r->height;
        r->band_stride = r->height ? r->height : 1;
    }
    // rows owned = sum over k of |[first + k*stride, +rows) intersect [0,height)|
    uint64_t rows = 0;
    for (uint64_t start = r->band_first; start < r->height; start += r->band_stride) {
        const uint64_t end = start + r->band_rows < r->height ? start + r->band_rows : r->height;
        rows += end - start;
    }
    r->local_rows = (uint32_t)rows;
    r->local_rows_padded = (r->local_rows + 7u) / 8u * 8u;
}

uint32_t ensure_iter_buffer(fs_renderer *r)
{
    // capacity is tracked in BYTES: the same frame needs twice the memory with IterType = uint64_t
    const size_t need = (size_t)r->w_block * 16u * r->local_rows_padded * r->iter_bytes;
    if (r->iters_external)
        return r->iters_external_bytes >= need ? 0 : (uint32_t)hipErrorInvalidValue; // never write past a caller's buffer
    if (r->iters_internal.p && r->iters_internal.cap >= need)
        return 0;
    if (r->iters_internal.p && r->display)
        FS_TRY(hipStreamSynchronize(r->display)); // a progressive RenderCurrent may still be reading it
    FS_TRY(buf_reserve(r, r->iters_internal, need, kFrame));
    if (r->compute)
        FS_TRY(hipStreamSynchronize(r->compute)); // usable from any stream from here on
    return 0;
}

void free_all(fs_renderer *r)
{
    free_perturb(r);
    exact_drop_kept(r);
    buf_release(r, r->iters_internal);
    (void)r_release(r, r->colors);
    (void)r_release(r, r->reduction);
    (void)r_release(r, r->stats);
    (void)r_release(r, r->queue);
    for (DevBuf *b : {&r->tile_probe, &r->tile_order, &r->lav2_cost, &r->lav2_order, &r->lav2_sort_tmp, &r->pix_cost, &r->at_res,
                      &r->at_cost, &r->at_order, &r->pix_order, &r->pix_work, &r->pix_temp, &r->cold_cost, &r->cold_order,
                      &r->cold_work, &r->cold_temp})
        buf_release(r, *b);
    // (a recorded order must not survive the buffer it indexes)
    r->at_order_valid = r->pix_valid = r->lav2_cost_valid = r->po_order_valid = false;
    // ... nor the palette's cache key the palette: the next fs_init_memory uploads again, whatever pointer and generation it
    // is given
    (void)r_release(r, r->pal);
    r->pal_cached_host = nullptr;
    r->pal_cached_gen = 0;
    r->pal_iters = 0;
    buf_release(r, r->cx_row);
    buf_release(r, r->arena);
    if (r->la_mail)
        (void)hipHostFree(r->la_mail);
    r->la_mail = nullptr;
    r->width = r->height = 0;
    release_kept_blocks(r);
}

} // namespace

extern "C" {

fs_renderer *fs_create(int device)
{
    fs_renderer *r = new (std::nothrow) fs_renderer();
    if (r) {
        r->device = device;
        // fault injection for the out-of-memory path (tests): every input-table allocation of this renderer behaves as if
        // the device were full and lands in page-locked host memory
        const char *e = getenv("FSMI355_FAIL_INPUT_ALLOC");
        r->inject_input_oom = e != nullptr && atoi(e) != 0;
        std::lock_guard<std::mutex> g(g_renderers_mu);
        g_renderers.push_back(r);
    }
    return r;
}

void fs_destroy(fs_renderer *r)
{
    if (!r)
        return;
    {
        std::lock_guard<std::mutex> g(g_renderers_mu);
        g_renderers.erase(std::remove(g_renderers.begin(), g_renderers.end(), r), g_renderers.end());
    }
    if (hipSetDevice(r->device) == hipSuccess) {
        if (r->compute)
            hipStreamSynchronize(r->compute);
        if (r->display)
            hipStreamSynchronize(r->display);
        free_all(r);
        if (r->compute)
            hipStreamSynchronize(r->compute); // the stream-ordered frees have run before their stream goes away
        for (uint32_t i = 0; i < fs_renderer::kTimingRing; i++) {
            if (r->ev_start[i])
                hipEventDestroy(r->ev_start[i]);
            if (r->ev_stop[i])
                hipEventDestroy(r->ev_stop[i]);
            if (r->ev_mid[i])
                hipEventDestroy(r->ev_mid[i]);
        }
        if (r->compute)
            hipStreamDestroy(r->compute);
        if (r->display)
            hipStreamDestroy(r->display);
    }
    delete r;
}

uint32_t fs_test_device_is_working(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return 0;
    // probe the caller's current device and leave it current (the reference hard-codes device 0 because it only ever
    // uses that one, GPU_Render.cu:113; a multi-GPU host has already selected its own)
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess || hipSetDevice(cur) != hipSuccess)
        return 0;
    if (hipFree(nullptr) != hipSuccess)
        return 0;
    return 1;
}

int fs_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0;
}

const char *fs_error_string(uint32_t err)
{
    switch (err) {
        case FS_OK:
            return "no error";
        case FS_ERR_1:
        case FS_ERR_2:
            return "FractalSharkError: unused";
        case FS_ERR_3:
            return "FractalSharkError::Error3: antialiasing must be 1..4";
        case FS_ERR_4:
            return "FractalSharkError::Error4: width not divisible by antialiasing";
        case FS_ERR_5:
            return "FractalSharkError::Error5: height not divisible by antialiasing";
        case FS_ERR_6:
            return "FractalSharkError::Error6: no uploaded orbit/table for this type";
        case FS_ERR_7:
            return "FractalSharkError::Error7";
        case FS_ERR_UNSUPPORTED:
            return "fsmi355: numeric type / mode not built into this library";
        default:
            return hipGetErrorString((hipError_t)err);
    }
}

uint32_t fs_init_memory(fs_renderer *r, uint32_t w, uint32_t h, uint32_t antialiasing, uint32_t iter_bytes,
                        const fs_color16 *pal_interleaved, uint32_t pal_iters, uint32_t palette_aux_depth,
                        uint64_t palette_generation, int expected_reuse)
{
    if (uint32_t e = use_device(r))
        return e;
    if (iter_bytes != 4 && iter_bytes != 8)
        return FS_ERR_UNSUPPORTED;
    exact_drop_kept(r);
    if (uint32_t e = ensure_streams(r))
        return e;
    // palette: re-upload when the host pointer or the generation changes (GPU_Render.cu:270-304)
    r->pal_aux_depth = palette_aux_depth;
    if (pal_interleaved && (r->pal_cached_host != pal_interleaved || r->pal_cached_gen != palette_generation ||
                            r->pal_iters != pal_iters)) {
        if (r->pal) {
            // a progressive RenderCurrent on the display stream may still be reading the old palette, and r_free parks the
            // block where the r_alloc below finds it again: the display stream must have drained before the block is reused
            // (hipFree used to synchronise the whole device here)
            FS_TRY(hipStreamSynchronize(r->display));
            FS_TRY(r_release(r, r->pal));
        }
        FS_TRY(r_alloc(r, (void **)&r->pal, sizeof(fs_color16) * (size_t)pal_iters, kFrame));
        FS_TRY(hipMemcpyAsync(r->pal, pal_interleaved, sizeof(fs_color16) * (size_t)pal_iters, hipMemcpyDefault,
                              r->compute));
        FS_TRY(hipStreamSynchronize(r->compute)); // host buffer is borrowed for the call only
        r->pal_iters = pal_iters;
        r->pal_cached_host = pal_interleaved;
        r->pal_cached_gen = palette_generation;
    }
    if (r->width == w && r->height == h && r->aa == antialiasing && r->iter_bytes == iter_bytes && expected_reuse)
        return 0;
    if (antialiasing > 4 || antialiasing < 1)
        return FS_ERR_3;
    if (w % antialiasing != 0)
        return FS_ERR_4;
    if (h % antialiasing != 0)
        return FS_ERR_5;

    r->w_block = w / 16 + (w % 16 != 0);
    r->h_block = h / 8 + (h % 8 != 0);
    r->width = w;
    r->height = h;
    r->aa = antialiasing;
    r->iter_bytes = iter_bytes;
    r->n_cu = (size_t)r->w_block * 16 * r->h_block * 8;
    r->color_w = w / antialiasing;
    r->color_h = h / antialiasing;
    const uint32_t wcb = r->color_w / 16 + (r->color_w % 16 != 0);
    const uint32_t hcb = r->color_h / 8 + (r->color_h % 8 != 0);
    r->n_color_cu = (size_t)wcb * 16 * hcb * 8;
    r->band_rows = 0;
    compute_local_rows(r);
    // a caller-owned iteration buffer was sized for the previous geometry: drop it (fs_set_external_iter_buffer again)
    r->iters_external = nullptr;
    r->iters_external_bytes = 0;

    // ResetMemory(..., ResetPerturb::Yes, ...) -- GPU_Render.cu:346.  Frees are ordered on the compute stream; the display
    // stream (progressive RenderCurrent) may still be reading the buffers that are about to go
    FS_TRY(hipStreamSynchronize(r->display));
    free_perturb(r);
    if (uint32_t e = ensure_iter_buffer(r)) {
        (void)hipGetLastError(); // reported by this return value, not by the launch check of a later frame
        free_all(r);
        return e;
    }
    (void)r_release(r, r->colors);
    if (!r->reduction)
        FS_TRY(r_alloc(r, (void **)&r->reduction, sizeof(fs_reduction), kFrame));
    if (!r->stats) {
        // 8 counters; a measurement build (FS_TRACE_WAVES) appends four words per wave of the largest frame it will see
        // (words 16..27: per-phase cycle counters of the FS_PROFILE_CYCLES build of the BLA kernel, tools/c5_phase_probe.py;
        // the two measurement builds are not combined)
        r->stats_words = 40; // (words 28..39: the probe build of k_lav2_hdr64's hand-written loops, tools/c4_arm_probe.py)
        if (const char *e = getenv("FSMI355_TRACE_WAVES"))
            r->stats_words = 16 + 4 * (size_t)atoll(e);
        FS_TRY(r_alloc(r, (void **)&r->stats, r->stats_words * sizeof(uint64_t), kFrame));
        FS_TRY(hipMemsetAsync(r->stats, 0, r->stats_words * sizeof(uint64_t), r->compute));
    }
    if (!r->queue)
        FS_TRY(r_alloc(r, (void **)&r->queue, 64, kFrame));
    FS_TRY(r_alloc(r, (void **)&r->colors, r->n_color_cu * sizeof(fs_color16), kFrame));
    if (uint32_t e = fs_clear(r))
        return e;
    // the frame buffers were allocated in compute-stream order; the display stream (and the caller's own streams, through
    // fs_device_iter_buffer) may use them from here on
    FS_TRY(hipStreamSynchronize(r->compute));
    return 0;
}

uint32_t fs_set_row_bands(fs_renderer *r, uint32_t band_first_row, uint32_t band_rows, uint32_t band_stride_rows)
{
    if (uint32_t e = use_device(r))
        return e;
    if (r->width == 0)
        return FS_ERR_6;
    if (band_rows != 0 && (band_stride_rows < band_rows))
        return FS_ERR_7;
    exact_drop_kept(r);
    r->band_first = band_first_row;
    r->band_rows = band_rows;
    r->band_stride = band_stride_rows;
    compute_local_rows(r);
    const uint32_t e = ensure_iter_buffer(r);
    if (e && r->iters_external) { // the caller's buffer does not hold the new banding: fall back to the internal one
        r->iters_external = nullptr;
        r->iters_external_bytes = 0;
        (void)ensure_iter_buffer(r);
    }
    return e;
}

uint32_t fs_local_rows(const fs_renderer *r) { return r->local_rows_padded; }

uint32_t fs_set_external_iter_buffer(fs_renderer *r, void *device_ptr, uint64_t capacity_bytes)
{
    if (uint32_t e = use_device(r))
        return e;
    if (r->width == 0)
        return FS_ERR_6;
    exact_drop_kept(r);
    r->iters_external = device_ptr;
    r->iters_external_bytes = device_ptr ? (size_t)capacity_bytes : 0;
    const uint32_t e = ensure_iter_buffer(r); // too small for the current geometry: rejected, internal buffer restored
    if (e && device_ptr) {
        r->iters_external = nullptr;
        r->iters_external_bytes = 0;
        (void)ensure_iter_buffer(r);
    }
    return e;
}

void *fs_device_iter_buffer(const fs_renderer *r) { return r->iters(); }

uint32_t fs_host_register(void *host_ptr, uint64_t bytes)
{
    return (uint32_t)hipHostRegister(host_ptr, (size_t)bytes, hipHostRegisterPortable);
}
uint32_t fs_host_unregister(void *host_ptr) { return (uint32_t)hipHostUnregister(host_ptr); }
uint32_t fs_rounded_width(const fs_renderer *r) { return r->w_block * 16u; }

uint32_t fs_sync_compute(fs_renderer *r)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->compute)
        return 0;
    return (uint32_t)hipStreamSynchronize(r->compute);
}

void *fs_compute_stream(const fs_renderer *r) { return (void *)r->compute; }
void *fs_display_stream(const fs_renderer *r) { return (void *)r->display; }

uint32_t fs_sync_display(fs_renderer *r)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->display)
        return 0;
    return (uint32_t)hipStreamSynchronize(r->display);
}

uint32_t fs_query_compute(fs_renderer *r)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->compute)
        return 0;
    return (uint32_t)hipStreamQuery(r->compute);
}

struct DoneThunk {
    fs_done_cb cb;
    void *user;
};

static void done_trampoline(void *p)
{
    DoneThunk *t = (DoneThunk *)p;
    t->cb(t->user);
    delete t;
}

uint32_t fs_enqueue_done_callback(fs_renderer *r, fs_done_cb cb, void *user)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!cb)
        return FS_ERR_6;
    DoneThunk *t = new DoneThunk{cb, user};
    // before InitializeMemory the reference's m_ComputeStream is the null stream and the callback still fires
    // (GPU_Render.cu:613-615); r->compute == nullptr behaves the same way
    const hipError_t e = hipLaunchHostFunc(r->compute, done_trampoline, t);
    if (e != hipSuccess)
        delete t;
    return (uint32_t)e;
}

uint64_t fs_host_fallback_bytes(const fs_renderer *r) { return r->host_alloc_bytes; }

uint64_t fs_idle_device_bytes(fs_renderer *r)
{
    std::lock_guard<std::mutex> g(r->kept_mu);
    uint64_t b = 0;
    for (const auto &k : r->kept_blocks)
        b += k.bytes;
    return b;
}

uint64_t fs_release_idle_device_memory(int device) { return release_idle_memory_of_device(device); }

uint32_t fs_get_width(const fs_renderer *r) { return r->width; }
uint32_t fs_get_height(const fs_renderer *r) { return r->height; }

float fs_last_kernel_ms(const fs_renderer *r)
{
    if (r->timed_launches == 0)
        return -1.0f;
    float ms = -1.0f;
    const uint32_t i = (uint32_t)((r->timed_launches - 1) % fs_renderer::kTimingRing);
    if (hipEventElapsedTime(&ms, r->ev_start[i], r->ev_stop[i]) != hipSuccess)
        return -1.0f;
    return ms;
}

uint32_t fs_kernel_ms_history(const fs_renderer *r, float *ms_out, uint32_t n)
{
    // the last n launches, oldest first; they must have completed (fs_sync_compute)
    if (n > fs_renderer::kTimingRing || n > r->timed_launches)
        return (uint32_t)hipErrorInvalidValue;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t i = (uint32_t)((r->timed_launches - n + k) % fs_renderer::kTimingRing);
        FS_TRY(hipEventElapsedTime(&ms_out[k], r->ev_start[i], r->ev_stop[i]));
    }
    return 0;
}

uint32_t fs_kernel_ms_split_history(const fs_renderer *r, float *first_ms, float *second_ms, uint32_t n)
{
    if (n > fs_renderer::kTimingRing || n > r->timed_launches)
        return (uint32_t)hipErrorInvalidValue;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t i = (uint32_t)((r->timed_launches - n + k) % fs_renderer::kTimingRing);
        if (r->mid_valid[i] && r->ev_mid[i]) {
            FS_TRY(hipEventElapsedTime(&first_ms[k], r->ev_start[i], r->ev_mid[i]));
            FS_TRY(hipEventElapsedTime(&second_ms[k], r->ev_mid[i], r->ev_stop[i]));
        } else {
            first_ms[k] = 0.0f;
            FS_TRY(hipEventElapsedTime(&second_ms[k], r->ev_start[i], r->ev_stop[i]));
        }
    }
    return 0;
}

} // extern "C"
