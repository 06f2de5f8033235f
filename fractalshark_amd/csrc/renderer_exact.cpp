#include "renderer_state.hpp"

#include "exact_atom_math.hpp"

using namespace fsr;

// ---- what the two exact paths (fs_render_exact: a lane per sample, fs_render_exact_wide: a wave per sample) share on the host.
// The device block of one call: [counter, statistics | cx | cy | `lists` lists of running samples], a list being the limb planes of
// x and y, then n, then the sample's id; with the cycle check (`cycle`) a list ends with the limb planes of the checkpoints, and
// the block with the byte plane of the proved samples (n_proved of them when that is not the lists' n: a continuation's lists hold
// the kept samples, its plane the frame).  With the period planes (`periods` pixels, fs_set_exact_periods; 0: none) the block goes on,
// per pixel: [2 * limbs limb planes of the smallest norm | its key | the atom period | with the cycle check, the cycle length];
// the kernels find them through an fsx::AtomPlanes in the block's head.  Point runs (`points`, fs_exact_eval_points; their period
// planes are per run) add behind those: [the runs' lengths | 2 * limbs limb planes of the endpoints].
struct ExactLayout {
    static constexpr size_t head = 256;
    uint32_t slots; // of a list
    bool cycle;
    size_t cx_bytes, cy_bytes, xy_bytes, n_bytes, id_bytes, list_bytes, proved_bytes;
    size_t min_bytes, plane_bytes; // the period planes: the minimum's limb planes, one uint64 plane; 0 without them
    size_t len_bytes, end_bytes;   // point runs: the lengths, the endpoints' limb planes; 0 without them
    ExactLayout(uint32_t limbs, uint32_t nx, uint32_t ny, uint32_t n, bool cycle_ = false, uint32_t n_proved = 0, uint32_t periods = 0,
                bool points = false)
        : slots(n), cycle(cycle_)
    {
        auto up = [](size_t b) { return (b + 255) / 256 * 256; };
        cx_bytes = up((size_t)limbs * nx * 4), cy_bytes = up((size_t)limbs * ny * 4);
        xy_bytes = up((size_t)2 * limbs * n * 4), n_bytes = up((size_t)n * 8), id_bytes = up((size_t)n * 4);
        list_bytes = xy_bytes + n_bytes + id_bytes + (cycle ? xy_bytes : 0);
        proved_bytes = cycle ? up(n_proved ? n_proved : n) : 0;
        min_bytes = periods ? up((size_t)2 * limbs * periods * 4) : 0, plane_bytes = periods ? up((size_t)periods * 8) : 0;
        len_bytes = points ? up((size_t)n * 8) : 0, end_bytes = points ? up((size_t)2 * limbs * n * 4) : 0;
    }
    size_t bytes(int lists) const
    {
        return head + cx_bytes + cy_bytes + (size_t)lists * list_bytes + proved_bytes + min_bytes + (cycle ? 3 : 2) * plane_bytes +
               len_bytes + end_bytes;
    }
    static constexpr size_t planes_at = 128; // (behind the counters and the statistics)
    fsx::AtomPlanes *period_planes(char *blk) const { return (fsx::AtomPlanes *)(blk + planes_at); }
    uint32_t *atom_min(char *blk, int lists) const { return (uint32_t *)(list_base(blk, lists) + proved_bytes); }
    // k = 0: the keys, 1: the atom periods, 2: the cycle lengths
    uint64_t *period_plane(char *blk, int lists, int k) const
    {
        return (uint64_t *)(list_base(blk, lists) + proved_bytes + min_bytes + (size_t)k * plane_bytes);
    }
    uint64_t *lengths(char *blk, int lists) const { return period_plane(blk, lists, cycle ? 3 : 2); }
    uint32_t *ends(char *blk, int lists) const { return (uint32_t *)((char *)lengths(blk, lists) + len_bytes); }
    // the parts of the list that starts at `base`
    FsExactList at(char *base) const
    {
        return {(uint32_t *)base, (uint64_t *)(base + xy_bytes), (uint32_t *)(base + xy_bytes + n_bytes),
                cycle ? (uint32_t *)(base + xy_bytes + n_bytes + id_bytes) : nullptr};
    }
    FsExactList list(char *blk, int k) const { return at(list_base(blk, k)); }
    uint8_t *proved(char *blk, int lists) const { return (uint8_t *)list_base(blk, lists); }
    uint32_t *count(char *blk) const { return (uint32_t *)blk; }
    uint32_t *park_count(char *blk) const { return (uint32_t *)(blk + 4); }
    unsigned long long *stats(char *blk) const { return (unsigned long long *)(blk + 16); }
    uint32_t *cx(char *blk) const { return (uint32_t *)(blk + head); }
    uint32_t *cy(char *blk) const { return (uint32_t *)(blk + head + cx_bytes); }

private:
    char *list_base(char *blk, int k) const { return blk + head + cx_bytes + cy_bytes + (size_t)k * list_bytes; }
};

// The kept set's block: the axes, ONE list of `samples` slots, the frame's proved plane.
ExactLayout fs_renderer::ExactKept::layout() const { return ExactLayout(limbs, W, H, samples, cycle, W * H); }

// ---- Keeping (fs_set_exact_keep, fs_render_exact_continue).  kExactKeep: the call parks the samples that meet the cap and leaves
// them as the renderer's kept set; kExactResume: the call starts from that set instead of z_1 = c (and keeps again).
enum ExactMode { kExactPlain = 0, kExactKeep = 1, kExactResume = 2 };

void fsr::exact_drop_kept(fs_renderer *r)
{
    if (r->exact.kept.blk)
        (void)r_free(r, r->exact.kept.blk);
    r->exact.kept = fs_renderer::ExactKept{};
}

// The kept set of a call that has just ended: the n_parked samples of `park` -- a list of the layout Ys -- repacked into a block
// of their size, with device copies of the axes and, with the check, the proved plane.  K: what the call was given; block and
// sample count are set here.  The set before it goes once the new one stands (a continuation's sources live in it).
static hipError_t exact_keep_install(fs_renderer *r, const ExactLayout &Ys, const FsExactList &park, uint32_t n_parked,
                                     const uint32_t *d_cx, const uint32_t *d_cy, const uint8_t *d_proved, fs_renderer::ExactKept K)
{
    hipStream_t s = r->compute;
    K.samples = n_parked;
    const uint32_t L = K.limbs, npix = K.W * K.H;
    const ExactLayout Yk = K.layout();
    char *nb = nullptr;
    hipError_t e = r_alloc(r, (void **)&nb, Yk.bytes(1), kFrame);
    if (e != hipSuccess)
        return e;
    e = hipMemcpyAsync(Yk.cx(nb), d_cx, (size_t)L * K.W * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(Yk.cy(nb), d_cy, (size_t)L * K.H * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && n_parked != 0) {
        // the 2L limb planes (and the checkpoint's 2L): rows of n_parked words, from a pitch of Ys.slots words to one of n_parked
        const FsExactList to = Yk.list(nb, 0);
        const size_t row = (size_t)n_parked * 4, pitch = (size_t)Ys.slots * 4;
        e = hipMemcpy2DAsync(to.xy, row, park.xy, pitch, row, 2 * L, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && K.cycle)
            e = hipMemcpy2DAsync(to.ck, row, park.ck, pitch, row, 2 * L, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(to.n, park.n, (size_t)n_parked * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(to.id, park.id, (size_t)n_parked * 4, hipMemcpyDeviceToDevice, s);
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
    K.blk = nb, K.valid = true;
    r->exact.kept = K;
    return hipSuccess;
}

// ---- The slice driver.  One run: a frame of the iteration buffer's geometry, or (W == 0; fs_exact_sample_counts, fs_exact_audit) n
// samples of their own, sample e at cx[l * n + e], cy[l * n + e] with nx == ny == n and `out` uint64 counts[n] on the device.
struct ExactPath;
struct ExactRun {
    const ExactPath *path;
    uint32_t frac_bits, limbs, bailout; // the number format
    int inclusive;
    const uint32_t *cx, *cy; // host axes, limb-major (kExactResume: not read, the kept set holds them)
    uint32_t nx, ny;         // values per axis
    uint32_t W;              // frame width; 0: samples
    uint32_t n;              // samples (kExactResume: the kept set's)
    void *out;               // device: counts
    uint32_t out_u64, out_pitch;
    uint64_t cap;
    bool cycle;              // the cycle check (lane path only): the C = true kernels run and the lists carry the checkpoints
    bool read_proved;        // with the check: the call's proved mask becomes the one fs_read_exact_proved returns
    bool periods;            // fs_render_exact with fs_set_exact_periods: the P = true kernels run and the period planes come back
    ExactMode mode;          // frames only
    // point runs (fs_exact_eval_points, fs_exact_eval_points_wide; samples on either path, no cycle check, nothing kept): run e
    // stops at lengths[e] instead of cap, the path's point-run kernels run (lane: S = true, P = true; wide: P = true), and the runs'
    // atom periods and endpoints (x planes, y planes: [limbs][n] each) go to the caller's host arrays -- not to the renderer's
    // planes, which stay the last frame's
    const uint64_t *lengths;
    uint64_t *atoms_out;
    uint32_t *end_x_out, *end_y_out;
};

static ExactRun exact_frame_run(const fs_renderer *r, const ExactPath &path, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx,
                                const uint32_t *cy, uint32_t bailout, int inclusive, uint64_t cap, void *out)
{
    ExactRun R{};
    R.path = &path, R.frac_bits = frac_bits, R.limbs = limbs, R.bailout = bailout, R.inclusive = inclusive;
    R.cx = cx, R.cy = cy, R.nx = r->width, R.ny = r->height, R.W = r->width, R.n = r->width * r->height;
    R.out = out, R.out_u64 = r->iter_bytes == 8 ? 1u : 0u, R.out_pitch = r->w_block * 16u;
    R.cap = cap;
    return R;
}

static ExactRun exact_sample_run(const ExactPath &path, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                                 uint32_t n, uint32_t bailout, int inclusive, uint64_t cap, uint64_t *out)
{
    ExactRun R{};
    R.path = &path, R.frac_bits = frac_bits, R.limbs = limbs, R.bailout = bailout, R.inclusive = inclusive;
    R.cx = cx, R.cy = cy, R.nx = R.ny = R.n = n;
    R.out = out, R.out_u64 = 1;
    R.cap = cap;
    return R;
}

// ---- What the slice driver is handed for each path: how a slice is launched, how long it is by default, and what the device
// statistics mean.  The driver describes a slice by the lane kernels' argument block; the wide launcher takes from it and from the
// run what its own block holds.
struct ExactPath {
    // false: nothing was launched, no kernel for the limb count
    bool (*launch)(const ExactRun &R, const FsExactArgs &A, bool cycle, bool keep, hipStream_t s);
    uint32_t (*default_slice)(uint32_t limbs, uint32_t n_src);
    void (*add_stats)(fs_renderer::Exact &X, const unsigned long long st[4]);
    bool fixed_slots; // fs_set_exact_slice's no_compaction applies
    bool wide;        // what fs_exact_kept_info reports of a set this path leaves
};

// The lane path (kernels_exact.hip, exact_math.hpp).
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
static void exact_add_stats(fs_renderer::Exact &X, const unsigned long long st[4])
{
    X.stats[0] += st[0], X.stats[1] += st[1];
    X.cycle_stats[0] += st[2], X.cycle_stats[1] += st[3];
}
static bool exact_lane_launch(const ExactRun &R, const FsExactArgs &A, bool cycle, bool keep, hipStream_t s)
{
    return fsk_exact_slice(A, R.limbs, R.W == 0, cycle, keep, R.periods || R.lengths, s);
}
static const ExactPath kExactLane = {exact_lane_launch, exact_default_slice, exact_add_stats, true, false};

// The wide path (kernels_exact_wide.hip).
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
static void wide_add_stats(fs_renderer::Exact &X, const unsigned long long st[4])
{
    X.stats[0] += 64ull * st[0], X.stats[1] += st[0]; // (the device counts the steps of a wave: 64 lane slots each)
}
// (no cycle check, no fixed slots and no resume flag here: a parked wide sample resumes as a running one)
static bool exact_wide_launch(const ExactRun &R, const FsExactArgs &A, bool, bool keep, hipStream_t s)
{
    FsExactWideArgs B{};
    B.cx = A.cx, B.cy = A.cy, B.nx = R.nx, B.ny = R.ny, B.W = R.W;
    B.out = R.out, B.out_u64 = R.out_u64, B.out_pitch = R.out_pitch;
    B.cap = A.cap, B.limbs = R.limbs, B.P = A.P;
    B.src = A.src, B.dst = A.dst, B.stride = A.stride, B.first = A.first, B.slice = A.slice;
    B.dst_count = A.dst_count, B.stats = A.stats, B.park_count = A.park_count;
    B.periods = A.periods, B.lengths = A.lengths;
    return fsk_exact_wide_slice(B, A.n_src, keep, R.lengths != nullptr, s);
}
static const ExactPath kExactWide = {exact_wide_launch, wide_default_slice, wide_add_stats, false, true};

struct ExactResult {
    uint32_t rc;
    bool touched; // false: the call returned before it touched the frame or the kept set (its one allocation failed)
};

// One device block per call: [counter, statistics | cx | cy | two lists of running samples | proved plane]; synchronous: the host
// reads the count of running samples after every slice.  Slice k reads lists[(k & 1) ^ 1] and writes the samples still running to
// lists[k & 1]; without compaction (ExactPath::fixed_slots) every slice works on the one list lists[fixed].
// kExactKeep parks the samples that meet the cap -- in the last slice's destination list, which no survivor is written to; without
// compaction in the other list -- and leaves them as the kept set.  kExactResume starts from the kept set: its list is the first
// slice's source and the second of the two lists from then on, the call's block [counter, statistics | one list] the other; axes
// and proved plane are the set's own, and the pixels proved so far take the new cap first.
static ExactResult exact_run(fs_renderer *r, const ExactRun &R)
{
    fs_renderer::Exact &X = r->exact;
    const ExactPath &P = *R.path;
    const bool keep = R.mode != kExactPlain, resume = R.mode == kExactResume, cycle = R.cycle;
    const fs_renderer::ExactKept K0 = X.kept;
    const uint32_t n = R.n, npix = R.W ? R.nx * R.ny : n;
    const bool points = R.lengths != nullptr;
    const bool periods = points || (R.periods && !keep && R.W != 0);
    const ExactLayout Y = resume ? K0.layout() : ExactLayout(R.limbs, R.nx, R.ny, n, cycle, npix, periods ? npix : 0, points);
    const bool compact = !(P.fixed_slots && X.no_compaction);
    const int n_lists = compact || keep ? 2 : 1;
    char *blk = nullptr;
    hipStream_t s = r->compute;
    hipError_t e = r_alloc(r, (void **)&blk, resume ? Y.head + Y.list_bytes : Y.bytes(n_lists), kFrame);
    if (e != hipSuccess)
        return {(uint32_t)e, false};
    // (without compaction the one list is lists[fixed]; the other, when there is one, is where the samples are parked)
    const int fixed = resume ? 1 : 0;
    const FsExactList lists[2] = {resume ? Y.at(blk + Y.head) : Y.list(blk, 0), resume ? Y.list(K0.blk, 0) : Y.list(blk, n_lists - 1)};
    char *axes = resume ? K0.blk : blk;

    FsExactArgs A{};
    A.cx = Y.cx(axes), A.cy = Y.cy(axes);
    A.W = R.nx, A.H = R.ny, A.rounded_width = R.out_pitch; // (samples: W == H == n, and no pitch)
    A.iter_u64 = R.out_u64, A.iters = R.out;
    A.cap = R.cap;
    A.P = fsx::make_params(R.frac_bits, R.bailout, R.inclusive);
    A.stride = n;
    A.n_src = n;
    A.first = resume ? 0u : 1u;
    A.resume = resume ? 1u : 0u;
    A.compact = compact ? 1u : 0u;
    A.dst_count = Y.count(blk);
    A.park_count = Y.park_count(blk);
    A.stats = Y.stats(blk);
    if (cycle) {
        A.proved = resume ? Y.proved(K0.blk, 1) : Y.proved(blk, n_lists);
        fsx::cycle_masks(X.cycle_fp_bits, A.fp_mx, A.fp_my);
    }
    static_assert(ExactLayout::planes_at + sizeof(fsx::AtomPlanes) <= ExactLayout::head && ExactLayout::planes_at >= 16 + 4 * 8, "the head");
    fsx::AtomPlanes planes{}; // (read by the copy below, which the first slice's synchronisation ends)
    if (periods) {
        planes.mn = Y.atom_min(blk, n_lists), planes.keys = Y.period_plane(blk, n_lists, 0);
        planes.atom = Y.period_plane(blk, n_lists, 1), planes.cyclen = cycle ? Y.period_plane(blk, n_lists, 2) : nullptr;
        planes.stride = npix;
        if (points)
            planes.end = Y.ends(blk, n_lists), A.lengths = Y.lengths(blk, n_lists);
        A.periods = Y.period_planes(blk);
        A.atom_key_shift = fsx::atom_key_shift(X.atom_key_bits);
    }

    e = hipMemsetAsync(blk, 0, Y.head, s);
    if (e == hipSuccess && cycle && !resume)
        e = hipMemsetAsync(A.proved, 0, npix, s);
    if (e == hipSuccess && periods) // (the atom plane and, behind it, the cycle lengths)
        e = hipMemsetAsync(planes.atom, 0, (cycle ? 2 : 1) * Y.plane_bytes, s);
    if (e == hipSuccess && periods)
        e = hipMemcpyAsync(Y.period_planes(blk), &planes, sizeof planes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && points)
        e = hipMemsetAsync(planes.end, 0, (size_t)2 * R.limbs * n * 4, s);
    if (e == hipSuccess && points)
        e = hipMemcpyAsync(Y.lengths(blk, n_lists), R.lengths, (size_t)n * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && resume && K0.proved != 0) { // (a sample the continuation proves writes the new cap itself)
        fsk_exact_set_proved(R.out, (int)R.out_u64, A.proved, R.nx, R.ny, R.out_pitch, R.cap, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess && !resume)
        e = hipMemcpyAsync(Y.cx(blk), R.cx, (size_t)R.limbs * R.nx * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !resume)
        e = hipMemcpyAsync(Y.cy(blk), R.cy, (size_t)R.limbs * R.ny * 4, hipMemcpyHostToDevice, s);

    // slice after slice until one leaves no sample running
    uint64_t slices = 0, after_first = 0;
    while (e == hipSuccess) {
        A.src = compact ? lists[(slices & 1) ^ 1] : lists[fixed], A.dst = compact ? lists[slices & 1] : lists[fixed];
        if (keep)
            A.park = compact ? A.dst : lists[fixed ^ 1];
        A.slice = X.slice ? X.slice : P.default_slice(R.limbs, A.n_src);
        uint32_t left = 0;
        e = hipMemsetAsync(A.dst_count, 0, sizeof(uint32_t), s);
        if (e == hipSuccess)
            e = P.launch(R, A, cycle, keep, s) ? hipGetLastError() : hipErrorInvalidValue;
        if (e == hipSuccess)
            e = hipMemcpyAsync(&left, A.dst_count, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (e != hipSuccess)
            break;
        if (slices++ == 0)
            after_first = left;
        if (left == 0)
            break;
        A.first = 0, A.resume = 0;
        if (compact)
            A.n_src = left;
    }

    unsigned long long st[4] = {0, 0, 0, 0};
    uint32_t n_parked = 0;
    if (e == hipSuccess)
        e = hipMemcpyAsync(st, A.stats, sizeof st, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && keep)
        e = hipMemcpyAsync(&n_parked, A.park_count, sizeof n_parked, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && cycle && R.read_proved) {
        X.proved.resize(npix);
        e = hipMemcpyAsync(X.proved.data(), A.proved, npix, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess && points) {
        e = hipMemcpyAsync(R.atoms_out, planes.atom, (size_t)n * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(R.end_x_out, planes.end, (size_t)R.limbs * n * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(R.end_y_out, planes.end + (size_t)R.limbs * n, (size_t)R.limbs * n * 4, hipMemcpyDeviceToHost, s);
    } else if (e == hipSuccess && periods) {
        X.atom.resize(npix);
        e = hipMemcpyAsync(X.atom.data(), planes.atom, (size_t)npix * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && cycle) {
            X.cyclen.resize(npix);
            e = hipMemcpyAsync(X.cyclen.data(), planes.cyclen, (size_t)npix * 8, hipMemcpyDeviceToHost, s);
        }
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (periods && !points)
        X.atom_valid = e == hipSuccess, X.cyclen_valid = cycle && e == hipSuccess;
    P.add_stats(X, st);
    X.stats[2] += slices, X.stats[3] += after_first;
    if (cycle && R.read_proved)
        X.proved_valid = e == hipSuccess;
    if (e == hipSuccess && keep) {
        fs_renderer::ExactKept K{};
        K.wide = P.wide, K.cycle = cycle, K.W = R.nx, K.H = R.ny, K.cap = R.cap;
        K.frac_bits = R.frac_bits, K.limbs = R.limbs, K.bailout = R.bailout, K.inclusive = R.inclusive ? 1 : 0;
        K.proved = (resume ? K0.proved : 0) + st[2];
        e = n_parked <= n ? exact_keep_install(r, Y, A.park, n_parked, A.cx, A.cy, A.proved, K) : hipErrorUnknown;
    }
    (void)r_free(r, blk);
    return {(uint32_t)e, true};
}

// fs_exact_wide_state: one launch of exactly `steps` steps on n samples of their own; every sample is written to the one list at
// its own slot, and the limb planes of x and y come back.  No loop, no statistics, no keeping.
static uint32_t exact_wide_state_run(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                                     uint32_t n, uint32_t steps, uint32_t *out_x, uint32_t *out_y)
{
    const ExactLayout Y(limbs, n, n, n);
    const size_t plane_bytes = (size_t)limbs * n * 4;
    char *blk = nullptr;
    hipStream_t s = r->compute;
    FS_TRY(r_alloc(r, (void **)&blk, Y.bytes(1), kFrame));
    FsExactWideArgs A{};
    A.cx = Y.cx(blk), A.cy = Y.cy(blk), A.nx = A.ny = n;
    A.limbs = limbs;
    // (a sample freezes at the bound the limb count is derived for: |z|^2 > 256 2^2F)
    A.P = fsx::make_params(frac_bits, fsx::kMaxBailout, 0);
    A.src = A.dst = Y.list(blk, 0);
    A.stride = n;
    A.first = 1, A.state_only = 1, A.slice = steps;
    A.dst_count = Y.count(blk), A.stats = Y.stats(blk); // (not written: no sample is counted, no step either)
    hipError_t e = hipMemsetAsync(blk, 0, Y.head, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(Y.cx(blk), cx, plane_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(Y.cy(blk), cy, plane_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = fsk_exact_wide_slice(A, n, false, false, s) ? hipGetLastError() : hipErrorInvalidValue;
    if (e == hipSuccess)
        e = hipMemcpyAsync(out_x, A.dst.xy, plane_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(out_y, A.dst.xy + (size_t)limbs * n, plane_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    (void)r_free(r, blk);
    return (uint32_t)e;
}

// ---- What the entry points refuse.  Each keeps the order its header lists; the pieces are these.
// The renderer has a frame (fs_init_memory) and holds all of its rows.
static bool exact_has_frame(const fs_renderer *r) { return r->memory_initialized() && r->compute; }
static uint32_t exact_frame_held(fs_renderer *r)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!exact_has_frame(r))
        return FS_ERR_6;
    if (r->local_rows != r->height)
        return FS_ERR_UNSUPPORTED; // this renderer holds some rows of the frame only
    return 0;
}

// the cap fits the frame's IterType
static bool exact_cap_fits(const fs_renderer *r, uint64_t n_iterations)
{
    return n_iterations != ~0ull && (n_iterations <= 0xFFFFFFFFull || r->iter_bytes == 8);
}

// the number format; max_limbs: fsx::kMaxLimbs for the lane kernels, fsw::kMaxLimbs for the wide ones.  The lane entry points have
// always summed frac_bits + 10 in 32 bits, so a frac_bits within 10 of 2^32 wraps past this test there; that stays as it is here.
static uint32_t exact_format_check(uint32_t frac_bits, uint32_t limbs, uint32_t max_limbs, uint32_t bailout)
{
    static_assert(fsx::kMinLimbs == fsw::kMinLimbs, "one floor for both paths");
    const uint64_t need = max_limbs == fsx::kMaxLimbs ? frac_bits + 10u : (uint64_t)frac_bits + 10u;
    if (limbs < fsx::kMinLimbs || limbs > max_limbs || 32ull * limbs < need || bailout < 1 || bailout > fsx::kMaxBailout)
        return FS_ERR_UNSUPPORTED;
    return 0;
}

// what fs_render_exact and fs_exact_stable_mask refuse first
static uint32_t exact_lane_begin(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, uint32_t bailout, uint64_t n_iterations)
{
    if (uint32_t e = exact_frame_held(r))
        return e;
    if (uint32_t e = exact_format_check(frac_bits, limbs, fsx::kMaxLimbs, bailout))
        return e;
    if (!exact_cap_fits(r, n_iterations) || (uint64_t)r->width * r->height > 0xFFFFFFFFull)
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
static bool exact_axes_in_range(const uint32_t *cx, uint32_t nx, const uint32_t *cy, uint32_t ny, uint32_t limbs, uint32_t frac_bits)
{
    return exact_axis_in_range(cx, nx, limbs, frac_bits) && exact_axis_in_range(cy, ny, limbs, frac_bits);
}

extern "C" {

// ---- fs_render_exact / fs_exact_stable_mask (the lane path)
uint32_t fs_set_exact_slice(fs_renderer *r, uint32_t steps, int no_compaction)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact.slice = steps;
    r->exact.no_compaction = no_compaction != 0;
    return 0;
}

uint32_t fs_read_exact_stats(const fs_renderer *r, uint64_t out[4])
{
    if (!r || !out)
        return hipErrorInvalidValue;
    memcpy(out, r->exact.stats, sizeof r->exact.stats);
    return 0;
}

uint32_t fs_set_exact_cycle_check(fs_renderer *r, int enable)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact.cycle_check = enable != 0;
    return 0;
}

uint32_t fs_set_exact_cycle_fingerprint_bits(fs_renderer *r, uint32_t bits)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact.cycle_fp_bits = bits;
    return 0;
}

uint32_t fs_read_exact_cycle_stats(const fs_renderer *r, uint64_t out[2])
{
    if (!r || !out)
        return hipErrorInvalidValue;
    memcpy(out, r->exact.cycle_stats, sizeof r->exact.cycle_stats);
    return 0;
}

uint32_t fs_read_exact_proved(const fs_renderer *r, uint8_t *out, uint64_t n)
{
    if (!r || !out)
        return hipErrorInvalidValue;
    if (!r->exact.proved_valid)
        return FS_ERR_6;
    if (n != r->exact.proved.size())
        return hipErrorInvalidValue;
    memcpy(out, r->exact.proved.data(), (size_t)n);
    return 0;
}

uint32_t fs_set_exact_periods(fs_renderer *r, int enable)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact.periods = enable != 0;
    return 0;
}

uint32_t fs_set_exact_atom_key_bits(fs_renderer *r, uint32_t bits)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact.atom_key_bits = bits;
    return 0;
}

static uint32_t exact_read_plane(const std::vector<uint64_t> &plane, bool valid, uint64_t *out, uint64_t n)
{
    if (!valid)
        return FS_ERR_6;
    if (n != plane.size())
        return hipErrorInvalidValue;
    memcpy(out, plane.data(), (size_t)n * 8);
    return 0;
}

uint32_t fs_read_exact_atom_periods(const fs_renderer *r, uint64_t *out, uint64_t n)
{
    if (!r || !out)
        return hipErrorInvalidValue;
    return exact_read_plane(r->exact.atom, r->exact.atom_valid, out, n);
}

uint32_t fs_read_exact_cycle_lengths(const fs_renderer *r, uint64_t *out, uint64_t n)
{
    if (!r || !out)
        return hipErrorInvalidValue;
    return exact_read_plane(r->exact.cyclen, r->exact.cyclen_valid, out, n);
}

uint32_t fs_render_exact(fs_renderer *r, uint32_t iter_bytes, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                         uint32_t bailout, int inclusive, uint64_t n_iterations)
{
    if (uint32_t e = exact_lane_begin(r, frac_bits, limbs, bailout, n_iterations))
        return e;
    // (fs_render_exact_wide looks at iter_bytes BEFORE the cap: the two disagree when both are wrong)
    if (iter_bytes != 4 && iter_bytes != 8)
        return FS_ERR_UNSUPPORTED;
    if (iter_bytes != r->iter_bytes || !cx || !cy)
        return (uint32_t)hipErrorInvalidValue;
    if (!exact_axes_in_range(cx, r->width, cy, r->height, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    if (r->exact.periods && r->exact.keep) // (a kept sample's minimum would have to travel with it: not built)
        return FS_ERR_UNSUPPORTED;
    r->exact.reset_stats();
    r->exact.atom_valid = r->exact.cyclen_valid = false;
    exact_drop_kept(r);
    ExactRun R = exact_frame_run(r, kExactLane, frac_bits, limbs, cx, cy, bailout, inclusive, n_iterations, r->iters());
    R.cycle = r->exact.cycle_check, R.read_proved = true, R.mode = r->exact.keep ? kExactKeep : kExactPlain;
    R.periods = r->exact.periods;
    return exact_run(r, R).rc;
}

uint32_t fs_exact_stable_mask(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *const cx[3], const uint32_t *const cy[3],
                              uint32_t bailout, uint64_t n_iterations, uint8_t *host_mask)
{
    if (uint32_t e = exact_lane_begin(r, frac_bits, limbs, bailout, n_iterations))
        return e;
    if (!cx || !cy || !host_mask)
        return (uint32_t)hipErrorInvalidValue;
    for (int k = 0; k < 3; k++) {
        if (!cx[k] || !cy[k])
            return (uint32_t)hipErrorInvalidValue;
        if (!exact_axes_in_range(cx[k], r->width, cy[k], r->height, limbs, frac_bits))
            return FS_ERR_UNSUPPORTED;
    }
    const uint32_t W = r->width, H = r->height, pitch = r->w_block * 16u;
    const size_t frame_bytes = ((size_t)pitch * r->local_rows_padded * r->iter_bytes + 255) / 256 * 256;
    char *blk = nullptr;
    FS_TRY(r_alloc(r, (void **)&blk, frame_bytes + (size_t)W * H, kFrame));
    uint8_t *d_mask = (uint8_t *)(blk + frame_bytes);
    r->exact.reset_stats(r->exact.cycle_check);
    uint32_t rc = 0;
    for (int d = 0; d < 4 && rc == 0; d++) { // c + s, c - s, c + is, c - is
        ExactRun R = exact_frame_run(r, kExactLane, frac_bits, limbs, d < 2 ? cx[1 + d] : cx[0], d < 2 ? cy[0] : cy[d - 1], bailout, 0,
                                     n_iterations, blk);
        R.cycle = r->exact.cycle_check;
        rc = exact_run(r, R).rc;
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

// ---- fs_exact_sample_counts / fs_render_exact_wide / fs_exact_wide_state (the wide path)
uint32_t fs_exact_sample_counts(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                                uint32_t n_samples, uint32_t bailout, int inclusive, uint64_t n_iterations, uint64_t *counts_out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (uint32_t e = exact_format_check(frac_bits, limbs, fsw::kMaxLimbs, bailout))
        return e;
    if (n_iterations == ~0ull)
        return (uint32_t)hipErrorInvalidValue;
    if (n_samples == 0)
        return 0;
    if (!cx || !cy || !counts_out || n_samples > kWideMaxSamples)
        return (uint32_t)hipErrorInvalidValue;
    if (!exact_axes_in_range(cx, n_samples, cy, n_samples, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    if (uint32_t e = ensure_streams(r)) // no fs_init_memory needed
        return e;
    uint64_t *d_out = nullptr;
    FS_TRY(r_alloc(r, (void **)&d_out, (size_t)n_samples * 8, kFrame));
    r->exact.reset_stats();
    uint32_t rc = exact_run(r, exact_sample_run(kExactWide, frac_bits, limbs, cx, cy, n_samples, bailout, inclusive, n_iterations, d_out)).rc;
    if (rc == 0)
        rc = (uint32_t)hipMemcpyAsync(counts_out, d_out, (size_t)n_samples * 8, hipMemcpyDeviceToHost, r->compute);
    if (rc == 0)
        rc = (uint32_t)hipStreamSynchronize(r->compute);
    (void)r_free(r, d_out);
    return rc;
}

uint32_t fs_exact_eval_points(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                              const uint64_t *lengths, uint32_t n_runs, uint32_t bailout, int inclusive, uint64_t *values_out,
                              uint64_t *atoms_out, uint32_t *end_x_out, uint32_t *end_y_out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (uint32_t e = exact_format_check(frac_bits, limbs, fsx::kMaxLimbs, bailout))
        return e;
    if (n_runs == 0)
        return 0;
    if (!cx || !cy || !lengths || !values_out || !atoms_out || !end_x_out || !end_y_out || n_runs > kWideMaxSamples)
        return (uint32_t)hipErrorInvalidValue;
    uint64_t longest = 0;
    for (uint32_t i = 0; i < n_runs; i++) {
        if (lengths[i] == 0 || lengths[i] == ~0ull)
            return (uint32_t)hipErrorInvalidValue;
        longest = lengths[i] > longest ? lengths[i] : longest;
    }
    if (!exact_axes_in_range(cx, n_runs, cy, n_runs, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    if (uint32_t e = ensure_streams(r)) // no fs_init_memory needed
        return e;
    uint64_t *d_out = nullptr;
    FS_TRY(r_alloc(r, (void **)&d_out, (size_t)n_runs * 8, kFrame));
    r->exact.reset_stats();
    // (the cycle-check, keep and periods switches are not read: no check, nothing kept, and the renderer's planes stay the frame's)
    ExactRun R = exact_sample_run(kExactLane, frac_bits, limbs, cx, cy, n_runs, bailout, inclusive, longest, d_out);
    R.lengths = lengths, R.atoms_out = atoms_out, R.end_x_out = end_x_out, R.end_y_out = end_y_out;
    uint32_t rc = exact_run(r, R).rc;
    if (rc == 0)
        rc = (uint32_t)hipMemcpyAsync(values_out, d_out, (size_t)n_runs * 8, hipMemcpyDeviceToHost, r->compute);
    if (rc == 0)
        rc = (uint32_t)hipStreamSynchronize(r->compute);
    (void)r_free(r, d_out);
    return rc;
}

// fs_exact_eval_points on the wide path: its checks in its order with 704 limbs in place of 24, its run with a wave per run
uint32_t fs_exact_eval_points_wide(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                                   const uint64_t *lengths, uint32_t n_runs, uint32_t bailout, int inclusive, uint64_t *values_out,
                                   uint64_t *atoms_out, uint32_t *end_x_out, uint32_t *end_y_out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (uint32_t e = exact_format_check(frac_bits, limbs, fsw::kMaxLimbs, bailout))
        return e;
    if (n_runs == 0)
        return 0;
    if (!cx || !cy || !lengths || !values_out || !atoms_out || !end_x_out || !end_y_out || n_runs > kWideMaxSamples)
        return (uint32_t)hipErrorInvalidValue;
    uint64_t longest = 0;
    for (uint32_t i = 0; i < n_runs; i++) {
        if (lengths[i] == 0 || lengths[i] == ~0ull)
            return (uint32_t)hipErrorInvalidValue;
        longest = lengths[i] > longest ? lengths[i] : longest;
    }
    if (!exact_axes_in_range(cx, n_runs, cy, n_runs, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    if (uint32_t e = ensure_streams(r)) // no fs_init_memory needed
        return e;
    uint64_t *d_out = nullptr;
    FS_TRY(r_alloc(r, (void **)&d_out, (size_t)n_runs * 8, kFrame));
    r->exact.reset_stats();
    // (the keep switch is not read either: nothing is kept, and the kept set stays what it was)
    ExactRun R = exact_sample_run(kExactWide, frac_bits, limbs, cx, cy, n_runs, bailout, inclusive, longest, d_out);
    R.lengths = lengths, R.atoms_out = atoms_out, R.end_x_out = end_x_out, R.end_y_out = end_y_out;
    uint32_t rc = exact_run(r, R).rc;
    if (rc == 0)
        rc = (uint32_t)hipMemcpyAsync(values_out, d_out, (size_t)n_runs * 8, hipMemcpyDeviceToHost, r->compute);
    if (rc == 0)
        rc = (uint32_t)hipStreamSynchronize(r->compute);
    (void)r_free(r, d_out);
    return rc;
}

uint32_t fs_render_exact_wide(fs_renderer *r, uint32_t iter_bytes, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx,
                              const uint32_t *cy, uint32_t bailout, int inclusive, uint64_t n_iterations)
{
    if (uint32_t e = exact_frame_held(r))
        return e;
    if (uint32_t e = exact_format_check(frac_bits, limbs, fsw::kMaxLimbs, bailout))
        return e;
    // (fs_render_exact looks at iter_bytes AFTER the cap: the two disagree when both are wrong)
    if (iter_bytes != 4 && iter_bytes != 8)
        return FS_ERR_UNSUPPORTED;
    if (!exact_cap_fits(r, n_iterations) || (uint64_t)r->width * r->height > kWideMaxSamples || iter_bytes != r->iter_bytes || !cx || !cy)
        return (uint32_t)hipErrorInvalidValue;
    if (!exact_axes_in_range(cx, r->width, cy, r->height, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    r->exact.reset_stats();
    exact_drop_kept(r);
    ExactRun R = exact_frame_run(r, kExactWide, frac_bits, limbs, cx, cy, bailout, inclusive, n_iterations, r->iters());
    R.mode = r->exact.keep ? kExactKeep : kExactPlain;
    return exact_run(r, R).rc;
}

uint32_t fs_exact_wide_state(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                             uint32_t n_samples, uint32_t steps, uint32_t *out_x, uint32_t *out_y)
{
    if (uint32_t e = use_device(r))
        return e;
    if (uint32_t e = exact_format_check(frac_bits, limbs, fsw::kMaxLimbs, 1))
        return e;
    if (n_samples == 0)
        return 0;
    if (!cx || !cy || !out_x || !out_y || n_samples > kWideMaxSamples)
        return (uint32_t)hipErrorInvalidValue;
    if (!exact_axes_in_range(cx, n_samples, cy, n_samples, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;
    if (uint32_t e = ensure_streams(r))
        return e;
    return exact_wide_state_run(r, frac_bits, limbs, cx, cy, n_samples, steps, out_x, out_y);
}

// ---- fs_set_exact_keep / fs_render_exact_continue / fs_exact_kept_info / fs_exact_drop_kept
uint32_t fs_set_exact_keep(fs_renderer *r, int enable)
{
    if (!r)
        return hipErrorInvalidValue;
    r->exact.keep = enable != 0;
    return 0;
}

uint32_t fs_exact_kept_info(const fs_renderer *r, fs_exact_kept *out)
{
    if (!r || !out)
        return hipErrorInvalidValue;
    memset(out, 0, sizeof *out);
    const fs_renderer::ExactKept &K = r->exact.kept;
    if (!K.valid)
        return 0;
    out->samples = K.samples, out->proved = K.proved, out->cap = K.cap, out->device_bytes = K.layout().bytes(1);
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
    fs_renderer::Exact &X = r->exact;
    fs_renderer::ExactKept &K = X.kept;
    if (!K.valid || !exact_has_frame(r) || K.W != r->width || K.H != r->height)
        return FS_ERR_6;
    if (!exact_cap_fits(r, n_iterations) || n_iterations < K.cap)
        return (uint32_t)hipErrorInvalidValue;
    if (n_iterations == K.cap)
        return 0;
    X.reset_stats();
    const uint32_t npix = K.W * K.H;
    if (K.samples == 0 && K.proved == 0) { // every pixel escaped: the frame of any cap, and with the check its all-zero mask
        if (K.cycle)
            X.proved.assign(npix, 0);
        X.proved_valid = K.cycle;
        K.cap = n_iterations;
        return 0;
    }
    if (K.samples == 0) { // nothing to resume: the proved pixels take the new cap, the plane stands, the cap moves
        hipStream_t s = r->compute;
        uint8_t *d_proved = K.layout().proved(K.blk, 1);
        fsk_exact_set_proved(r->iters(), r->iter_bytes == 8, d_proved, K.W, K.H, r->w_block * 16u, n_iterations, s);
        uint32_t rc = (uint32_t)hipGetLastError();
        if (rc == 0) {
            X.proved.resize(npix);
            rc = (uint32_t)hipMemcpyAsync(X.proved.data(), d_proved, npix, hipMemcpyDeviceToHost, s);
        }
        if (rc == 0)
            rc = (uint32_t)hipStreamSynchronize(s);
        X.proved_valid = rc == 0;
        K.cap = n_iterations;
        if (rc != 0)
            exact_drop_kept(r);
        return rc;
    }
    // (the axes are the set's own; a failure before the call touched the frame or the set leaves both standing)
    ExactRun R = exact_frame_run(r, K.wide ? kExactWide : kExactLane, K.frac_bits, K.limbs, nullptr, nullptr, K.bailout, K.inclusive,
                                 n_iterations, r->iters());
    R.n = K.samples, R.cycle = K.cycle, R.read_proved = true, R.mode = kExactResume;
    const ExactResult res = exact_run(r, R);
    if (res.rc != 0 && res.touched)
        exact_drop_kept(r);
    return res.rc;
}

// ---- fs_exact_audit: the host side (kernels_exact.hip's sample mode or kernels_exact_wide.hip, then kernels_exact_audit.hip).
// The runs of a call are one list: run k of sample i is entry k * n_samples + i, so limb plane l of the list is the caller's
// cx_runs[k][l][..] for k = 0, 1, ... side by side.  One device block per call: [record | xs | ys | counts | exact | frame |
// stable_bits]; the slices' own block comes and goes inside exact_run.
uint32_t fs_exact_audit(fs_renderer *r, const void *device_iters, uint32_t frac_bits, uint32_t limbs, const uint32_t *xs,
                        const uint32_t *ys, uint32_t n_samples, uint32_t n_levels, const uint32_t *cx_runs, const uint32_t *cy_runs,
                        uint32_t bailout, int inclusive, uint64_t n_iterations, fs_audit_result *out, uint64_t *exact_out,
                        uint64_t *frame_out, uint32_t *stable_out)
{
    if (uint32_t e = exact_frame_held(r))
        return e;
    if (uint32_t e = exact_format_check(frac_bits, limbs, fsw::kMaxLimbs, bailout))
        return e;
    if (n_levels > FS_AUDIT_MAX_LEVELS)
        return FS_ERR_UNSUPPORTED;
    if (!out || !exact_cap_fits(r, n_iterations))
        return (uint32_t)hipErrorInvalidValue;
    memset(out, 0, sizeof *out);
    r->exact.reset_stats();
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
    if (!exact_axes_in_range(cx.data(), n_runs, cy.data(), n_runs, limbs, frac_bits))
        return FS_ERR_UNSUPPORTED;

    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t rec_bytes = up(sizeof(fs_audit_result)), pos_bytes = up((size_t)n_samples * 4), cnt_bytes = up((size_t)n_runs * 8),
                 v_bytes = up((size_t)n_samples * 8);
    char *blk = nullptr;
    hipStream_t s = r->compute;
    FS_TRY(r_alloc(r, (void **)&blk, rec_bytes + 3 * pos_bytes + cnt_bytes + 2 * v_bytes, kFrame));
    FsAuditArgs A{};
    A.iters = device_iters ? device_iters : r->iters();
    A.iter_u64 = r->iter_bytes == 8 ? 1u : 0u, A.pitch = r->w_block * 16u;
    A.out = (fs_audit_result *)blk;
    A.xs = (const uint32_t *)(blk + rec_bytes), A.ys = (const uint32_t *)(blk + rec_bytes + pos_bytes);
    A.counts = (const uint64_t *)(blk + rec_bytes + 2 * pos_bytes);
    A.exact = (uint64_t *)(blk + rec_bytes + 2 * pos_bytes + cnt_bytes), A.frame = A.exact + v_bytes / 8;
    A.stable = (uint32_t *)(blk + rec_bytes + 2 * pos_bytes + cnt_bytes + 2 * v_bytes);
    A.n_samples = n_samples, A.n_levels = n_levels, A.cap = n_iterations;

    uint32_t rc = (uint32_t)hipMemcpyAsync((void *)A.xs, xs, (size_t)n_samples * 4, hipMemcpyHostToDevice, s);
    if (rc == 0)
        rc = (uint32_t)hipMemcpyAsync((void *)A.ys, ys, (size_t)n_samples * 4, hipMemcpyHostToDevice, s);
    if (rc == 0) {
        const bool lane = limbs <= fsx::kMaxLimbs;
        ExactRun R = exact_sample_run(lane ? kExactLane : kExactWide, frac_bits, limbs, cx.data(), cy.data(), n_runs, bailout, inclusive,
                                      n_iterations, (uint64_t *)A.counts);
        R.cycle = lane && r->exact.cycle_check, R.read_proved = true;
        rc = exact_run(r, R).rc;
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
