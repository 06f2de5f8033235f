#include "renderer_state.hpp"

#include "exact_cycle_math.hpp"

using namespace fsr;

// ---- what the two exact paths (fs_render_exact: a lane per sample, fs_render_exact_wide: a wave per sample) share on the host.
// The device block of one call: [counter, statistics | cx | cy | `lists` lists of running samples], a list being the limb planes of
// x and y, then n, then the sample's id; with the cycle check (`cycle`) a list ends with the limb planes of the checkpoints, and
// the block with the byte plane of the proved samples (n_proved of them when that is not the lists' n: a continuation's lists hold
// the kept samples, its plane the frame).
struct ExactLayout {
    static constexpr size_t head = 256;
    size_t cx_bytes, cy_bytes, xy_bytes, n_bytes, id_bytes, list_bytes, proved_bytes;
    ExactLayout(uint32_t limbs, uint32_t nx, uint32_t ny, uint32_t n, bool cycle = false, uint32_t n_proved = 0)
    {
        auto up = [](size_t b) { return (b + 255) / 256 * 256; };
        cx_bytes = up((size_t)limbs * nx * 4), cy_bytes = up((size_t)limbs * ny * 4);
        xy_bytes = up((size_t)2 * limbs * n * 4), n_bytes = up((size_t)n * 8), id_bytes = up((size_t)n * 4);
        list_bytes = xy_bytes + n_bytes + id_bytes + (cycle ? xy_bytes : 0);
        proved_bytes = cycle ? up(n_proved ? n_proved : n) : 0;
    }
    size_t bytes(int lists) const { return head + cx_bytes + cy_bytes + (size_t)lists * list_bytes + proved_bytes; }
    uint32_t *checkpoints(char *list) const { return (uint32_t *)(list + xy_bytes + n_bytes + id_bytes); }
    uint8_t *proved(char *blk, int lists) const { return (uint8_t *)list(blk, lists); }
    uint32_t *count(char *blk) const { return (uint32_t *)blk; }
    uint32_t *park_count(char *blk) const { return (uint32_t *)(blk + 4); }
    unsigned long long *stats(char *blk) const { return (unsigned long long *)(blk + 16); }
    uint32_t *cx(char *blk) const { return (uint32_t *)(blk + head); }
    uint32_t *cy(char *blk) const { return (uint32_t *)(blk + head + cx_bytes); }
    char *list(char *blk, int k) const { return blk + head + cx_bytes + cy_bytes + (size_t)k * list_bytes; }
};

// Slice after slice until one leaves no sample running.  launch(k) starts slice k on the stream (false: nothing was launched, the
// limb count has no kernel); survivors(left) hears how many samples slice k left running before slice k + 1 is set up.  The host
// reads that count after every slice, so the loop is synchronous.
template <class Launch, class Survivors>
static hipError_t exact_slice_loop(hipStream_t s, uint32_t *d_cnt, Launch launch, Survivors survivors, uint64_t &slices,
                                   uint64_t &after_first)
{
    for (;;) {
        uint32_t left = 0;
        hipError_t e = hipMemsetAsync(d_cnt, 0, sizeof(uint32_t), s);
        if (e != hipSuccess)
            return e;
        if (!launch(slices))
            return hipErrorInvalidValue;
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(&left, d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (e != hipSuccess)
            return e;
        if (slices++ == 0)
            after_first = left;
        if (left == 0)
            return hipSuccess;
        survivors(left);
    }
}

// ---- Keeping (fs_set_exact_keep, fs_render_exact_continue).  kExactKeep: the call parks the samples that meet the cap and leaves
// them as the renderer's kept set; kExactResume: the call starts from that set instead of z_1 = c (and keeps again).
enum ExactMode { kExactPlain = 0, kExactKeep = 1, kExactResume = 2 };

void fsr::exact_drop_kept(fs_renderer *r)
{
    if (r->exact_kept.blk)
        (void)r_free(r, r->exact_kept.blk);
    r->exact_kept = fs_renderer::ExactKept{};
}

// The kept set of a call that has just ended: the n_parked samples of `park` -- a list of the layout Ys with src_stride slots --
// repacked into a block of their size, with device copies of the axes and, with the check, the proved plane.  K: what the call was
// given; block, size and sample count are set here.  The set before it goes once the new one stands (a continuation's sources
// live in it).
static hipError_t exact_keep_install(fs_renderer *r, const ExactLayout &Ys, char *park, uint32_t src_stride, uint32_t n_parked,
                                     const uint32_t *d_cx, const uint32_t *d_cy, const uint8_t *d_proved, fs_renderer::ExactKept K)
{
    hipStream_t s = r->compute;
    const uint32_t L = K.limbs, npix = K.W * K.H;
    const ExactLayout Yk(L, K.W, K.H, n_parked, K.cycle, npix);
    char *nb = nullptr;
    hipError_t e = r_alloc(r, (void **)&nb, Yk.bytes(1), kFrame);
    if (e != hipSuccess)
        return e;
    e = hipMemcpyAsync(Yk.cx(nb), d_cx, (size_t)L * K.W * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(Yk.cy(nb), d_cy, (size_t)L * K.H * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && n_parked != 0) {
        // the 2L limb planes (and the checkpoint's 2L): rows of n_parked words, from a pitch of src_stride words to one of n_parked
        char *dl = Yk.list(nb, 0);
        const size_t row = (size_t)n_parked * 4;
        e = hipMemcpy2DAsync(dl, row, park, (size_t)src_stride * 4, row, 2 * L, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && K.cycle)
            e = hipMemcpy2DAsync(Yk.checkpoints(dl), row, Ys.checkpoints(park), (size_t)src_stride * 4, row, 2 * L,
                                 hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dl + Yk.xy_bytes, park + Ys.xy_bytes, (size_t)n_parked * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dl + Yk.xy_bytes + Yk.n_bytes, park + Ys.xy_bytes + Ys.n_bytes, (size_t)n_parked * 4,
                               hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess && K.cycle)
        e = hipMemcpyAsync(Yk.proved(nb, 1), d_proved, npix, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)r_free(r, nb);
        return e;
    }
    exact_drop_kept(r);
    K.blk = nb, K.bytes = Yk.bytes(1), K.samples = n_parked, K.valid = true;
    r->exact_kept = K;
    return hipSuccess;
}

extern "C" {

// ---- fs_render_exact / fs_exact_stable_mask: the host side (kernels_exact.hip, exact_math.hpp).
// Steps per lane per launch: at most 4096 -- one wave's pace with 24 limbs is 11.7 us per step, 48 ms a launch --
// and fewer when the list is long enough to fill the chip several times over: the chip sustains 5.6e9 lane steps per second with 24
// limbs and about (24 / L)^2 times that with L, so 1.5e11 / L^2 lane steps per launch keep a launch near 50 ms at any frame size and
// limb count.  As the compaction shortens the list the slices grow back to 4096.  Never under 64: a launch is not worth less.
static constexpr uint32_t kExactSlice = 4096, kExactSliceMin = 64;
static uint32_t exact_default_slice(uint32_t limbs, uint32_t n_src)
{
    const uint64_t k = (uint64_t)(1.5e11 / ((double)limbs * limbs)) / (n_src ? n_src : 1u);
    return (uint32_t)(k > kExactSlice ? kExactSlice : k < kExactSliceMin ? kExactSliceMin : k);
}

uint32_t fs_set_exact_slice(fs_renderer *r, uint32_t steps, int no_compaction)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact_slice = steps;
    r->exact_no_compaction = no_compaction != 0;
    return 0;
}

uint32_t fs_read_exact_stats(const fs_renderer *r, uint64_t out[4])
{
    if (!r || !out)
        return hipErrorInvalidValue;
    memcpy(out, r->exact_stats, sizeof r->exact_stats);
    return 0;
}

uint32_t fs_set_exact_cycle_check(fs_renderer *r, int enable)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact_cycle_check = enable != 0;
    return 0;
}

uint32_t fs_set_exact_cycle_fingerprint_bits(fs_renderer *r, uint32_t bits)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact_cycle_fp_bits = bits;
    return 0;
}

uint32_t fs_read_exact_cycle_stats(const fs_renderer *r, uint64_t out[2])
{
    if (!r || !out)
        return hipErrorInvalidValue;
    memcpy(out, r->exact_cycle_stats, sizeof r->exact_cycle_stats);
    return 0;
}

uint32_t fs_read_exact_proved(const fs_renderer *r, uint8_t *out, uint64_t n)
{
    if (!r || !out)
        return hipErrorInvalidValue;
    if (!r->exact_proved_valid)
        return FS_ERR_6;
    if (n != r->exact_proved.size())
        return hipErrorInvalidValue;
    memcpy(out, r->exact_proved.data(), (size_t)n);
    return 0;
}

// What every exact entry point does to the statistics before it starts.  keep_proved: the call leaves the mask of
// fs_read_exact_proved as it is (the shifted frames of fs_exact_stable_mask with the check on).
static void exact_reset_stats(fs_renderer *r, bool keep_proved = false)
{
    memset(r->exact_stats, 0, sizeof r->exact_stats);
    memset(r->exact_cycle_stats, 0, sizeof r->exact_cycle_stats);
    if (!keep_proved)
        r->exact_proved_valid = false;
}

// What both entry points refuse, in the order the header lists it.
static uint32_t exact_begin(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, uint32_t bailout, uint64_t n_iterations)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->memory_initialized() || !r->compute)
        return FS_ERR_6;
    if (r->local_rows != r->height)
        return FS_ERR_UNSUPPORTED; // this renderer holds some rows of the frame only
    if (limbs < fsx::kMinLimbs || limbs > fsx::kMaxLimbs || 32u * limbs < frac_bits + 10u || bailout < 1 ||
        bailout > fsx::kMaxBailout)
        return FS_ERR_UNSUPPORTED;
    if ((n_iterations > 0xFFFFFFFFull && r->iter_bytes != 8) || n_iterations == ~0ull ||
        (uint64_t)r->width * r->height > 0xFFFFFFFFull)
        return (uint32_t)hipErrorInvalidValue;
    return 0;
}

// every value of a limb-major axis (n values of `limbs` limbs) in [-32 * 2^F, 32 * 2^F): bits F + 5 and up all equal the sign
static bool exact_axis_in_range(const uint32_t *axis, uint32_t n, uint32_t limbs, uint32_t frac_bits)
{
    const uint32_t lo = frac_bits + fsx::kCBoundLog2;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t ext = 0u - (axis[(size_t)(limbs - 1) * n + i] >> 31);
        for (uint32_t l = lo / 32; l < limbs; l++) {
            const uint32_t mask = l == lo / 32 ? ~0u << (lo % 32) : ~0u;
            if ((axis[(size_t)l * n + i] ^ ext) & mask)
                return false;
        }
    }
    return true;
}

// One exact frame into `out` (a buffer of the iteration buffer's geometry).  One device block per call: [counter, statistics | cx |
// cy | two lists of running samples]; synchronous.  n_runs != 0 (fs_exact_audit): a list of n_runs runs of their own instead of a
// frame, cx and cy holding n_runs values each and `out` uint64 counts[n_runs] on the device (the kernel's sample mode).
// With the cycle check on (fs_set_exact_cycle_check) the C = true kernels run and the lists carry the checkpoints; keep_proved:
// the call's proved mask becomes the one fs_read_exact_proved returns.
// mode (frames only): kExactKeep parks the samples that meet the cap -- in the last slice's destination list, which no survivor is
// written to; without compaction in a second list -- and leaves them as the kept set.  kExactResume starts from the kept set (cx,
// cy and the format arguments are not read: the set's hold): its list is the first slice's source and the second of the two lists
// from then on, the call's block [counter, statistics | one list] the other; axes and proved plane are the set's own, and the
// pixels proved so far take the new cap first.  *started (when given) = false when the call returns before it has touched the frame
// or the set: its one allocation failed.
static uint32_t exact_frame(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                            uint32_t bailout, int inclusive, uint64_t n_iterations, void *out, uint32_t n_runs = 0,
                            bool keep_proved = false, ExactMode mode = kExactPlain, bool *started = nullptr)
{
    if (started)
        *started = false;
    const bool samples = n_runs != 0, keep = mode != kExactPlain, resume = mode == kExactResume;
    const fs_renderer::ExactKept K0 = r->exact_kept;
    if (resume)
        frac_bits = K0.frac_bits, limbs = K0.limbs, bailout = K0.bailout, inclusive = K0.inclusive;
    const bool cycle = resume ? K0.cycle : r->exact_cycle_check;
    const uint32_t W = samples ? n_runs : r->width, H = samples ? n_runs : r->height, npix = samples ? n_runs : W * H;
    const uint32_t n_list = resume ? K0.samples : npix; // slots of a list
    const ExactLayout Y(limbs, W, H, n_list, cycle, npix);
    const bool compact = !r->exact_no_compaction;
    const int n_lists = compact || keep ? 2 : 1;
    char *blk = nullptr;
    hipStream_t s = r->compute;
    FS_TRY(r_alloc(r, (void **)&blk, resume ? Y.head + Y.list_bytes : Y.bytes(n_lists), kFrame));
    if (started)
        *started = true;
    unsigned long long *d_stats = Y.stats(blk);
    // (without compaction the one list is lists[fixed]; the other, when there is one, is where the samples are parked)
    const int fixed = resume ? 1 : 0;
    char *lists[2] = {resume ? blk + Y.head : Y.list(blk, 0), resume ? Y.list(K0.blk, 0) : Y.list(blk, n_lists - 1)};
    char *axes = resume ? K0.blk : blk, *park = nullptr;

    FsExactArgs A{};
    A.cx = Y.cx(axes), A.cy = Y.cy(axes);
    A.W = W, A.H = H, A.rounded_width = samples ? 0u : r->w_block * 16u;
    A.iter_u64 = samples || r->iter_bytes == 8 ? 1u : 0u;
    A.iters = out;
    A.cap = n_iterations;
    A.P = fsx::make_params(frac_bits, bailout, inclusive);
    A.stride = n_list;
    A.n_src = n_list;
    A.first = resume ? 0u : 1u;
    A.resume = resume ? 1u : 0u;
    A.compact = compact ? 1u : 0u;
    A.dst_count = Y.count(blk);
    A.park_count = Y.park_count(blk);
    A.stats = d_stats;
    if (cycle) {
        A.proved = resume ? Y.proved(K0.blk, 1) : Y.proved(blk, n_lists);
        fsx::cycle_masks(r->exact_cycle_fp_bits, A.fp_mx, A.fp_my);
    }

    uint64_t slices = 0, after_first = 0;
    hipError_t e = hipMemsetAsync(blk, 0, Y.head, s);
    if (e == hipSuccess && cycle && !resume)
        e = hipMemsetAsync(A.proved, 0, npix, s);
    if (e == hipSuccess && resume && K0.proved != 0) { // (a sample the continuation proves writes the new cap itself)
        fsk_exact_set_proved(out, r->iter_bytes == 8, A.proved, W, H, r->w_block * 16u, n_iterations, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess && !resume)
        e = hipMemcpyAsync(Y.cx(blk), cx, (size_t)limbs * W * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !resume)
        e = hipMemcpyAsync(Y.cy(blk), cy, (size_t)limbs * H * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = exact_slice_loop(
            s, A.dst_count,
            [&](uint64_t k) {
                char *src = compact ? lists[(k & 1) ^ 1] : lists[fixed], *dst = compact ? lists[k & 1] : lists[fixed];
                if (keep) {
                    park = compact ? dst : lists[fixed ^ 1];
                    A.park_xy = (uint32_t *)park, A.park_n = (uint64_t *)(park + Y.xy_bytes);
                    A.park_pix = (uint32_t *)(park + Y.xy_bytes + Y.n_bytes), A.park_ck = Y.checkpoints(park);
                }
                A.src_xy = (const uint32_t *)src, A.src_n = (const uint64_t *)(src + Y.xy_bytes);
                A.src_pix = (const uint32_t *)(src + Y.xy_bytes + Y.n_bytes);
                A.dst_xy = (uint32_t *)dst, A.dst_n = (uint64_t *)(dst + Y.xy_bytes), A.dst_pix = (uint32_t *)(dst + Y.xy_bytes + Y.n_bytes);
                if (cycle)
                    A.src_ck = Y.checkpoints(src), A.dst_ck = Y.checkpoints(dst);
                A.slice = r->exact_slice ? r->exact_slice : exact_default_slice(limbs, A.n_src);
                return fsk_exact_slice(A, limbs, samples, cycle, keep, s);
            },
            [&](uint32_t left) {
                A.first = 0, A.resume = 0;
                if (compact)
                    A.n_src = left;
            },
            slices, after_first);
    unsigned long long st[4] = {0, 0, 0, 0};
    uint32_t n_parked = 0;
    if (e == hipSuccess)
        e = hipMemcpyAsync(st, d_stats, sizeof st, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && keep)
        e = hipMemcpyAsync(&n_parked, A.park_count, sizeof n_parked, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && cycle && keep_proved) {
        r->exact_proved.resize(npix);
        e = hipMemcpyAsync(r->exact_proved.data(), A.proved, npix, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    r->exact_stats[0] += st[0], r->exact_stats[1] += st[1], r->exact_stats[2] += slices, r->exact_stats[3] += after_first;
    r->exact_cycle_stats[0] += st[2], r->exact_cycle_stats[1] += st[3];
    if (cycle && keep_proved)
        r->exact_proved_valid = e == hipSuccess;
    if (e == hipSuccess && keep) {
        fs_renderer::ExactKept K = K0; // (a continuation: the set's own parameters)
        K.wide = false, K.cycle = cycle, K.W = W, K.H = H, K.cap = n_iterations;
        K.frac_bits = frac_bits, K.limbs = limbs, K.bailout = bailout, K.inclusive = inclusive ? 1 : 0;
        K.proved = (resume ? K0.proved : 0) + st[2];
        e = n_parked <= n_list ? exact_keep_install(r, Y, park, n_list, n_parked, A.cx, A.cy, A.proved, K) : hipErrorUnknown;
    }
    (void)r_free(r, blk);
    return (uint32_t)e;
}

uint32_t fs_render_exact(fs_renderer *r, uint32_t iter_bytes, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                         uint32_t bailout, int inclusive, uint64_t n_iterations)
{
    if (uint32_t e = exact_begin(r, frac_bits, limbs, bailout, n_iterations))
        return e;
    if (iter_bytes != 4 && iter_bytes != 8)
        return FS_ERR_UNSUPPORTED;
    if (iter_bytes != r->iter_bytes || !cx || !cy)
        return (uint32_t)hipErrorInvalidValue;
    if (!exact_axis_in_range(cx, r->width, limbs, frac_bits) || !exact_axis_in_range(cy, r->height, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    exact_reset_stats(r);
    exact_drop_kept(r);
    return exact_frame(r, frac_bits, limbs, cx, cy, bailout, inclusive, n_iterations, r->iters(), 0, true,
                       r->exact_keep ? kExactKeep : kExactPlain);
}

uint32_t fs_exact_stable_mask(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *const cx[3], const uint32_t *const cy[3],
                              uint32_t bailout, uint64_t n_iterations, uint8_t *host_mask)
{
    if (uint32_t e = exact_begin(r, frac_bits, limbs, bailout, n_iterations))
        return e;
    if (!cx || !cy || !host_mask)
        return (uint32_t)hipErrorInvalidValue;
    for (int k = 0; k < 3; k++) {
        if (!cx[k] || !cy[k])
            return (uint32_t)hipErrorInvalidValue;
        if (!exact_axis_in_range(cx[k], r->width, limbs, frac_bits) || !exact_axis_in_range(cy[k], r->height, limbs, frac_bits))
            return FS_ERR_UNSUPPORTED;
    }
    const uint32_t W = r->width, H = r->height, pitch = r->w_block * 16u;
    const size_t frame_bytes = ((size_t)pitch * r->local_rows_padded * r->iter_bytes + 255) / 256 * 256;
    char *blk = nullptr;
    FS_TRY(r_alloc(r, (void **)&blk, frame_bytes + (size_t)W * H, kFrame));
    uint8_t *d_mask = (uint8_t *)(blk + frame_bytes);
    exact_reset_stats(r, r->exact_cycle_check);
    uint32_t rc = 0;
    for (int d = 0; d < 4 && rc == 0; d++) { // c + s, c - s, c + is, c - is
        rc = exact_frame(r, frac_bits, limbs, d < 2 ? cx[1 + d] : cx[0], d < 2 ? cy[0] : cy[d - 1], bailout, 0, n_iterations, blk);
        if (rc == 0) {
            fsk_exact_mask(r->iters(), blk, r->iter_bytes == 8, d_mask, W, H, pitch, d == 0, r->compute);
            rc = (uint32_t)hipGetLastError();
        }
    }
    if (rc == 0)
        rc = (uint32_t)hipMemcpyAsync(host_mask, d_mask, (size_t)W * H, hipMemcpyDeviceToHost, r->compute);
    if (rc == 0)
        rc = (uint32_t)hipStreamSynchronize(r->compute);
    (void)r_free(r, blk);
    return rc;
}

// ---- fs_exact_sample_counts / fs_render_exact_wide / fs_exact_wide_state: the host side (kernels_exact_wide.hip).
// Steps per launch.  A lone wave's step takes wide_step_ns(L): 1.5 us plus, for each of its ceil(L / M) rounds, 16.7 M^2 + 36 M + 133 ns
// (M = limbs per lane) -- the fit of DESIGN.md 6.3 "Wide" to the measured pace, through M = 1, 2 and 11 and within 4 % at M = 3
// and 5.  The chip runs 1024 waves -- one per SIMD -- at that pace and shares the SIMDs among more (at 11 limbs per lane exactly
// so; at few limbs per lane it does better, and the launches come out shorter), so a list of n samples advances at
// ceil(n / 1024) times the lone step time.  K = 50 ms over that, never under 16 steps.
static constexpr uint32_t kWideMaxSamples = 0x7FFFFFFFu; // one workgroup per sample: the grid's x dimension
static constexpr uint32_t kWideSliceMin = 16, kWideSliceMax = 1u << 20, kWideWavesAtOnce = 1024;
static double wide_step_ns(uint32_t limbs)
{
    const uint32_t m = fsw::block_for(limbs);
    const double M = (double)m, nb = (double)((limbs + m - 1) / m);
    return 1500.0 + nb * (16.7 * M * M + 36.0 * M + 133.0);
}
static uint32_t wide_default_slice(uint32_t limbs, uint32_t n_src)
{
    const double passes = (double)((n_src + kWideWavesAtOnce - 1) / kWideWavesAtOnce);
    const double k = 50e6 / (wide_step_ns(limbs) * (passes < 1 ? 1 : passes));
    return k > kWideSliceMax ? kWideSliceMax : k < kWideSliceMin ? kWideSliceMin : (uint32_t)k;
}

// what every wide entry point refuses about the number format
static uint32_t wide_check(uint32_t frac_bits, uint32_t limbs, uint32_t bailout)
{
    if (limbs < fsw::kMinLimbs || limbs > fsw::kMaxLimbs || 32ull * limbs < (uint64_t)frac_bits + 10u || bailout < 1 ||
        bailout > fsx::kMaxBailout)
        return FS_ERR_UNSUPPORTED;
    return 0;
}

struct WideJob {
    uint32_t frac_bits, limbs;
    const uint32_t *cx, *cy;
    uint32_t nx, ny;     // values per axis
    uint32_t W;          // 0: samples (nx == ny == n)
    uint32_t n;          // samples
    uint32_t bailout;
    int inclusive;
    uint64_t cap;
    void *out;           // device: counts
    uint32_t out_u64, out_pitch;
    uint32_t state_steps; // fs_exact_wide_state: steps to apply, and ...
    uint32_t *state_x, *state_y; // ... host arrays [limbs][n] for the result
    bool state_only;
};

// One device block per call: [counter, statistics | cx | cy | two lists of running samples]; synchronous.
// mode (frames only), as exact_frame's: kExactKeep parks the samples that meet the cap in the last slice's destination list and
// leaves them as the kept set; kExactResume starts from the kept set (J.n = its samples; J.cx and J.cy are not read), whose list is
// the second of the two lists, the call's block [counter, statistics | one list] the first.  *started as exact_frame's.
static uint32_t exact_wide_run(fs_renderer *r, const WideJob &J, ExactMode mode = kExactPlain, bool *started = nullptr)
{
    if (started)
        *started = false;
    const bool keep = mode != kExactPlain, resume = mode == kExactResume;
    const fs_renderer::ExactKept K0 = r->exact_kept;
    const uint32_t L = J.limbs, n = J.n;
    const ExactLayout Y(L, J.nx, J.ny, n);
    char *blk = nullptr;
    hipStream_t s = r->compute;
    FS_TRY(r_alloc(r, (void **)&blk, resume ? Y.head + Y.list_bytes : Y.bytes(2), kFrame));
    if (started)
        *started = true;
    unsigned long long *d_stats = Y.stats(blk);
    char *lists[2] = {resume ? blk + Y.head : Y.list(blk, 0), resume ? Y.list(K0.blk, 0) : Y.list(blk, 1)};
    char *axes = resume ? K0.blk : blk, *park = nullptr;

    FsExactWideArgs A{};
    A.cx = Y.cx(axes), A.cy = Y.cy(axes);
    A.nx = J.nx, A.ny = J.ny, A.W = J.W;
    A.out = J.out, A.out_u64 = J.out_u64, A.out_pitch = J.out_pitch;
    A.cap = J.cap;
    A.limbs = L;
    // (the state call freezes a sample at the bound the limb count is derived for: |z|^2 > 256 2^2F)
    A.P = J.state_only ? fsx::make_params(J.frac_bits, fsx::kMaxBailout, 0) : fsx::make_params(J.frac_bits, J.bailout, J.inclusive);
    A.stride = n;
    A.first = resume ? 0u : 1u;
    A.state_only = J.state_only ? 1u : 0u;
    A.dst_count = Y.count(blk);
    A.park_count = Y.park_count(blk);
    A.stats = d_stats;

    uint32_t n_src = n;
    uint64_t slices = 0, after_first = 0;
    auto set_lists = [&](uint64_t k) {
        char *src = lists[(k & 1) ^ 1], *dst = lists[k & 1];
        park = dst;
        A.src_xy = (const uint32_t *)src, A.src_n = (const uint64_t *)(src + Y.xy_bytes);
        A.src_id = (const uint32_t *)(src + Y.xy_bytes + Y.n_bytes);
        A.dst_xy = (uint32_t *)dst, A.dst_n = (uint64_t *)(dst + Y.xy_bytes), A.dst_id = (uint32_t *)(dst + Y.xy_bytes + Y.n_bytes);
    };
    hipError_t e = hipMemsetAsync(blk, 0, Y.head, s);
    if (e == hipSuccess && !resume)
        e = hipMemcpyAsync(Y.cx(blk), J.cx, (size_t)L * J.nx * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !resume)
        e = hipMemcpyAsync(Y.cy(blk), J.cy, (size_t)L * J.ny * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && J.state_only) {
        // one launch of exactly state_steps steps; every sample is written to list 0 at its own slot
        set_lists(0);
        A.slice = J.state_steps;
        e = fsk_exact_wide_slice(A, n, false, s) ? hipGetLastError() : hipErrorInvalidValue;
        if (e == hipSuccess)
            e = hipMemcpyAsync(J.state_x, Y.list(blk, 0), (size_t)L * n * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(J.state_y, Y.list(blk, 0) + (size_t)L * n * 4, (size_t)L * n * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
    } else if (e == hipSuccess) {
        e = exact_slice_loop(
            s, A.dst_count,
            [&](uint64_t k) {
                set_lists(k);
                A.slice = r->exact_slice ? r->exact_slice : wide_default_slice(L, n_src);
                return fsk_exact_wide_slice(A, n_src, keep, s);
            },
            [&](uint32_t left) {
                A.first = 0;
                n_src = left;
            },
            slices, after_first);
    }
    unsigned long long st = 0;
    uint32_t n_parked = 0;
    if (e == hipSuccess)
        e = hipMemcpyAsync(&st, d_stats, sizeof st, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && keep)
        e = hipMemcpyAsync(&n_parked, A.park_count, sizeof n_parked, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    r->exact_stats[0] += 64ull * st, r->exact_stats[1] += st, r->exact_stats[2] += slices, r->exact_stats[3] += after_first;
    if (e == hipSuccess && keep) {
        fs_renderer::ExactKept K{};
        K.wide = true, K.cycle = false, K.W = J.nx, K.H = J.ny, K.cap = J.cap;
        K.frac_bits = J.frac_bits, K.limbs = L, K.bailout = J.bailout, K.inclusive = J.inclusive ? 1 : 0;
        e = n_parked <= n ? exact_keep_install(r, Y, park, n, n_parked, A.cx, A.cy, nullptr, K) : hipErrorUnknown;
    }
    (void)r_free(r, blk);
    return (uint32_t)e;
}

uint32_t fs_exact_sample_counts(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                                uint32_t n_samples, uint32_t bailout, int inclusive, uint64_t n_iterations, uint64_t *counts_out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (uint32_t e = wide_check(frac_bits, limbs, bailout))
        return e;
    if (n_iterations == ~0ull)
        return (uint32_t)hipErrorInvalidValue;
    if (n_samples == 0)
        return 0;
    if (!cx || !cy || !counts_out || n_samples > kWideMaxSamples)
        return (uint32_t)hipErrorInvalidValue;
    if (!exact_axis_in_range(cx, n_samples, limbs, frac_bits) || !exact_axis_in_range(cy, n_samples, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    if (uint32_t e = ensure_streams(r)) // no fs_init_memory needed
        return e;
    uint64_t *d_out = nullptr;
    FS_TRY(r_alloc(r, (void **)&d_out, (size_t)n_samples * 8, kFrame));
    exact_reset_stats(r);
    WideJob J{};
    J.frac_bits = frac_bits, J.limbs = limbs, J.cx = cx, J.cy = cy, J.nx = J.ny = J.n = n_samples, J.W = 0;
    J.bailout = bailout, J.inclusive = inclusive, J.cap = n_iterations;
    J.out = d_out, J.out_u64 = 1;
    uint32_t rc = exact_wide_run(r, J);
    if (rc == 0)
        rc = (uint32_t)hipMemcpyAsync(counts_out, d_out, (size_t)n_samples * 8, hipMemcpyDeviceToHost, r->compute);
    if (rc == 0)
        rc = (uint32_t)hipStreamSynchronize(r->compute);
    (void)r_free(r, d_out);
    return rc;
}

uint32_t fs_render_exact_wide(fs_renderer *r, uint32_t iter_bytes, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx,
                              const uint32_t *cy, uint32_t bailout, int inclusive, uint64_t n_iterations)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->memory_initialized() || !r->compute)
        return FS_ERR_6;
    if (r->local_rows != r->height)
        return FS_ERR_UNSUPPORTED; // this renderer holds some rows of the frame only
    if (uint32_t e = wide_check(frac_bits, limbs, bailout))
        return e;
    if (iter_bytes != 4 && iter_bytes != 8)
        return FS_ERR_UNSUPPORTED;
    if ((n_iterations > 0xFFFFFFFFull && r->iter_bytes != 8) || n_iterations == ~0ull ||
        (uint64_t)r->width * r->height > kWideMaxSamples || iter_bytes != r->iter_bytes || !cx || !cy)
        return (uint32_t)hipErrorInvalidValue;
    if (!exact_axis_in_range(cx, r->width, limbs, frac_bits) || !exact_axis_in_range(cy, r->height, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    exact_reset_stats(r);
    WideJob J{};
    J.frac_bits = frac_bits, J.limbs = limbs, J.cx = cx, J.cy = cy, J.nx = r->width, J.ny = r->height, J.W = r->width;
    J.n = r->width * r->height;
    J.bailout = bailout, J.inclusive = inclusive, J.cap = n_iterations;
    J.out = r->iters(), J.out_u64 = r->iter_bytes == 8 ? 1u : 0u, J.out_pitch = r->w_block * 16u;
    exact_drop_kept(r);
    return exact_wide_run(r, J, r->exact_keep ? kExactKeep : kExactPlain);
}

// ---- fs_set_exact_keep / fs_render_exact_continue / fs_exact_kept_info / fs_exact_drop_kept
uint32_t fs_set_exact_keep(fs_renderer *r, int enable)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact_keep = enable != 0;
    return 0;
}

uint32_t fs_exact_kept_info(const fs_renderer *r, fs_exact_kept *out)
{
    if (!r || !out)
        return hipErrorInvalidValue;
    memset(out, 0, sizeof *out);
    const fs_renderer::ExactKept &K = r->exact_kept;
    if (!K.valid)
        return 0;
    out->samples = K.samples, out->proved = K.proved, out->cap = K.cap, out->device_bytes = K.bytes;
    out->frac_bits = K.frac_bits, out->limbs = K.limbs, out->bailout = K.bailout, out->inclusive = (uint32_t)K.inclusive;
    out->wide = K.wide ? 1u : 0u, out->cycle_check = K.cycle ? 1u : 0u, out->valid = 1u;
    return 0;
}

uint32_t fs_exact_drop_kept(fs_renderer *r)
{
    if (!r)
        return hipErrorInvalidValue;
    if (uint32_t e = use_device(r))
        return e;
    exact_drop_kept(r);
    return 0;
}

uint32_t fs_render_exact_continue(fs_renderer *r, uint64_t n_iterations)
{
    if (!r)
        return hipErrorInvalidValue;
    if (uint32_t e = use_device(r))
        return e;
    fs_renderer::ExactKept &K = r->exact_kept;
    if (!K.valid || !r->memory_initialized() || !r->compute || K.W != r->width || K.H != r->height)
        return FS_ERR_6;
    if (n_iterations == ~0ull || n_iterations < K.cap || (n_iterations > 0xFFFFFFFFull && r->iter_bytes != 8))
        return (uint32_t)hipErrorInvalidValue;
    if (n_iterations == K.cap)
        return 0;
    exact_reset_stats(r);
    const uint32_t npix = K.W * K.H;
    if (K.samples == 0 && K.proved == 0) { // every pixel escaped: the frame of any cap, and with the check its all-zero mask
        if (K.cycle)
            r->exact_proved.assign(npix, 0);
        r->exact_proved_valid = K.cycle;
        K.cap = n_iterations;
        return 0;
    }
    hipStream_t s = r->compute;
    uint32_t rc = 0;
    bool started = true; // (false: the call failed before it touched the frame or the set, which then stands)
    if (K.samples != 0) {
        if (K.wide) {
            WideJob J{};
            J.frac_bits = K.frac_bits, J.limbs = K.limbs, J.nx = K.W, J.ny = K.H, J.W = K.W, J.n = K.samples;
            J.bailout = K.bailout, J.inclusive = K.inclusive, J.cap = n_iterations;
            J.out = r->iters(), J.out_u64 = r->iter_bytes == 8 ? 1u : 0u, J.out_pitch = r->w_block * 16u;
            rc = exact_wide_run(r, J, kExactResume, &started);
        } else {
            rc = exact_frame(r, 0, 0, nullptr, nullptr, 0, 0, n_iterations, r->iters(), 0, true, kExactResume, &started);
        }
    } else { // nothing to resume: the proved pixels take the new cap, the plane stands, the cap moves
        const ExactLayout Y(K.limbs, K.W, K.H, K.samples, K.cycle, npix);
        fsk_exact_set_proved(r->iters(), r->iter_bytes == 8, Y.proved(K.blk, 1), K.W, K.H, r->w_block * 16u, n_iterations, s);
        rc = (uint32_t)hipGetLastError();
        if (rc == 0) {
            r->exact_proved.resize(npix);
            rc = (uint32_t)hipMemcpyAsync(r->exact_proved.data(), Y.proved(K.blk, 1), npix, hipMemcpyDeviceToHost, s);
        }
        if (rc == 0)
            rc = (uint32_t)hipStreamSynchronize(s);
        r->exact_proved_valid = rc == 0;
        K.cap = n_iterations;
    }
    if (rc != 0 && started)
        exact_drop_kept(r);
    return rc;
}

uint32_t fs_exact_wide_state(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                             uint32_t n_samples, uint32_t steps, uint32_t *out_x, uint32_t *out_y)
{
    if (uint32_t e = use_device(r))
        return e;
    if (uint32_t e = wide_check(frac_bits, limbs, 1))
        return e;
    if (n_samples == 0)
        return 0;
    if (!cx || !cy || !out_x || !out_y || n_samples > kWideMaxSamples)
        return (uint32_t)hipErrorInvalidValue;
    if (!exact_axis_in_range(cx, n_samples, limbs, frac_bits) || !exact_axis_in_range(cy, n_samples, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    if (uint32_t e = ensure_streams(r))
        return e;
    WideJob J{};
    J.frac_bits = frac_bits, J.limbs = limbs, J.cx = cx, J.cy = cy, J.nx = J.ny = J.n = n_samples, J.W = 0;
    J.state_only = true, J.state_steps = steps, J.state_x = out_x, J.state_y = out_y;
    const uint64_t keep[4] = {r->exact_stats[0], r->exact_stats[1], r->exact_stats[2], r->exact_stats[3]};
    const uint32_t rc = exact_wide_run(r, J);
    memcpy(r->exact_stats, keep, sizeof keep);
    return rc;
}

// ---- fs_exact_audit: the host side (kernels_exact.hip's sample mode or kernels_exact_wide.hip, then kernels_exact_audit.hip).
// The runs of a call are one list: run k of sample i is entry k * n_samples + i, so limb plane l of the list is the caller's
// cx_runs[k][l][..] for k = 0, 1, ... side by side.  One device block per call: [record | xs | ys | counts | exact | frame |
// stable_bits]; the slices' own block comes and goes inside exact_frame / exact_wide_run.
uint32_t fs_exact_audit(fs_renderer *r, const void *device_iters, uint32_t frac_bits, uint32_t limbs, const uint32_t *xs,
                        const uint32_t *ys, uint32_t n_samples, uint32_t n_levels, const uint32_t *cx_runs, const uint32_t *cy_runs,
                        uint32_t bailout, int inclusive, uint64_t n_iterations, fs_audit_result *out, uint64_t *exact_out,
                        uint64_t *frame_out, uint32_t *stable_out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->memory_initialized() || !r->compute)
        return FS_ERR_6;
    if (r->local_rows != r->height)
        return FS_ERR_UNSUPPORTED; // this renderer holds some rows of the frame only
    if (uint32_t e = wide_check(frac_bits, limbs, bailout))
        return e;
    if (n_levels > FS_AUDIT_MAX_LEVELS)
        return FS_ERR_UNSUPPORTED;
    if (!out || (n_iterations > 0xFFFFFFFFull && r->iter_bytes != 8) || n_iterations == ~0ull)
        return (uint32_t)hipErrorInvalidValue;
    memset(out, 0, sizeof *out);
    exact_reset_stats(r);
    if (n_samples == 0)
        return 0;
    const uint32_t runs_per_sample = 1u + 4u * n_levels;
    const uint64_t n_runs64 = (uint64_t)n_samples * runs_per_sample;
    if (!xs || !ys || !cx_runs || !cy_runs || n_runs64 > kWideMaxSamples)
        return (uint32_t)hipErrorInvalidValue;
    for (uint32_t i = 0; i < n_samples; i++)
        if (xs[i] >= r->width || ys[i] >= r->height)
            return (uint32_t)hipErrorInvalidValue;
    const uint32_t n_runs = (uint32_t)n_runs64;
    // limb plane l of the list: run k's plane l behind run k - 1's
    std::vector<uint32_t> cx((size_t)limbs * n_runs), cy((size_t)limbs * n_runs);
    for (uint32_t k = 0; k < runs_per_sample; k++)
        for (uint32_t l = 0; l < limbs; l++) {
            const size_t src = ((size_t)k * limbs + l) * n_samples, dst = (size_t)l * n_runs + (size_t)k * n_samples;
            memcpy(&cx[dst], cx_runs + src, (size_t)n_samples * 4);
            memcpy(&cy[dst], cy_runs + src, (size_t)n_samples * 4);
        }
    if (!exact_axis_in_range(cx.data(), n_runs, limbs, frac_bits) || !exact_axis_in_range(cy.data(), n_runs, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;

    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t rec_bytes = up(sizeof(fs_audit_result)), xy_bytes = up((size_t)n_samples * 4), cnt_bytes = up((size_t)n_runs * 8),
                 v_bytes = up((size_t)n_samples * 8);
    char *blk = nullptr;
    hipStream_t s = r->compute;
    FS_TRY(r_alloc(r, (void **)&blk, rec_bytes + 3 * xy_bytes + cnt_bytes + 2 * v_bytes, kFrame));
    FsAuditArgs A{};
    A.iters = device_iters ? device_iters : r->iters();
    A.iter_u64 = r->iter_bytes == 8 ? 1u : 0u, A.pitch = r->w_block * 16u;
    A.out = (fs_audit_result *)blk;
    A.xs = (const uint32_t *)(blk + rec_bytes), A.ys = (const uint32_t *)(blk + rec_bytes + xy_bytes);
    A.counts = (const uint64_t *)(blk + rec_bytes + 2 * xy_bytes);
    A.exact = (uint64_t *)(blk + rec_bytes + 2 * xy_bytes + cnt_bytes), A.frame = A.exact + v_bytes / 8;
    A.stable = (uint32_t *)(blk + rec_bytes + 2 * xy_bytes + cnt_bytes + 2 * v_bytes);
    A.n_samples = n_samples, A.n_levels = n_levels, A.cap = n_iterations;

    uint32_t rc = (uint32_t)hipMemcpyAsync((void *)A.xs, xs, (size_t)n_samples * 4, hipMemcpyHostToDevice, s);
    if (rc == 0)
        rc = (uint32_t)hipMemcpyAsync((void *)A.ys, ys, (size_t)n_samples * 4, hipMemcpyHostToDevice, s);
    if (rc == 0) {
        if (limbs <= fsx::kMaxLimbs) {
            rc = exact_frame(r, frac_bits, limbs, cx.data(), cy.data(), bailout, inclusive, n_iterations, (void *)A.counts, n_runs,
                             true);
        } else {
            WideJob J{};
            J.frac_bits = frac_bits, J.limbs = limbs, J.cx = cx.data(), J.cy = cy.data(), J.nx = J.ny = J.n = n_runs, J.W = 0;
            J.bailout = bailout, J.inclusive = inclusive, J.cap = n_iterations;
            J.out = (void *)A.counts, J.out_u64 = 1;
            rc = exact_wide_run(r, J);
        }
    }
    if (rc == 0) {
        fsk_exact_audit(A, s);
        rc = (uint32_t)hipGetLastError();
    }
    if (rc == 0)
        rc = (uint32_t)hipMemcpyAsync(out, A.out, sizeof *out, hipMemcpyDeviceToHost, s);
    if (rc == 0 && exact_out)
        rc = (uint32_t)hipMemcpyAsync(exact_out, A.exact, (size_t)n_samples * 8, hipMemcpyDeviceToHost, s);
    if (rc == 0 && frame_out)
        rc = (uint32_t)hipMemcpyAsync(frame_out, A.frame, (size_t)n_samples * 8, hipMemcpyDeviceToHost, s);
    if (rc == 0 && stable_out)
        rc = (uint32_t)hipMemcpyAsync(stable_out, A.stable, (size_t)n_samples * 4, hipMemcpyDeviceToHost, s);
    const uint32_t rs = (uint32_t)hipStreamSynchronize(s); // (also when something failed: the copies above read the caller's arrays)
    (void)r_free(r, blk);
    return rc ? rc : rs;
}

} // extern "C"
