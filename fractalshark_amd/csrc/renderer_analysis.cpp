// renderer_analysis.cpp -- what looks at a frame or at candidates instead of rendering: the Feature Finder evaluators and the
// autozoom pick.
#include "renderer_state.hpp"

#include <algorithm>
#include <cmath>

#include "autozoom_math.hpp"
#include "feature_plain.hpp"

using namespace fsr;

// Steps per candidate per launch of the Feature Finder evaluator (kernels_feature.hip): bounds one launch to a fraction of a
// second at the measured pace, whatever the iteration cap.
static constexpr uint32_t kFeatureSlice = 1u << 18;

// seq: the resident orbit is its waypoints (fs_feature_eval_resident); the lane records then carry a cursor each.
template <class F>
static uint32_t feature_eval(fs_renderer *r, uint32_t iter_bytes, int mode, const void *radius, uint64_t max_iters,
                             const void *in, void *out, uint64_t n, bool seq = false)
{
    using In = typename FsFeatRec<F>::In;
    using Out = typename FsFeatRec<F>::Out;
    using Real = typename FsDev<F>::Real;
    const auto *zref = (const typename FsDev<F>::Z *)(sizeof(F) == 4 ? (const void *)r->zref : (const void *)r->zref64);
    const auto *c_low = (const Real *)(sizeof(F) == 4 ? (const void *)r->c_low32 : (const void *)r->c_low64);
    if (iter_bytes == 4 && mode == FS_FEATURE_FIXED)
        for (uint64_t k = 0; k < n; k++)
            if (((const In *)in)[k].period > 0xFFFFFFFFull)
                return hipErrorInvalidValue; // a period IterType cannot hold
    const Real rad = *(const Real *)radius;
    const fs::hreal<F> R{rad.m, rad.e};
    hipStream_t s = r->compute;
    void *d_in = nullptr, *d_out = nullptr, *d_st = nullptr, *d_cnt = nullptr;
    hipError_t e = r_alloc(r, &d_in, n * sizeof(In), kFrame);
    if (e == hipSuccess)
        e = r_alloc(r, &d_out, n * sizeof(Out), kFrame);
    if (e == hipSuccess)
        e = r_alloc(r, &d_st, n * (seq ? fsk_feature_seq_lane_bytes<F>(iter_bytes == 8) : sizeof(FsFeatLane<F>)), kFrame);
    if (e == hipSuccess)
        e = r_alloc(r, &d_cnt, sizeof(uint32_t), kFrame);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_in, in, n * sizeof(In), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        if (seq)
            fsk_feature_seq_init<F>(d_in, d_st, d_out, n, mode == FS_FEATURE_FIND, R, max_iters, r->orbit_uncompressed, r->wp_raw,
                                    (uint32_t)r->orbit_size, iter_bytes == 8, s);
        else
            fsk_feature_init<F>(d_in, (FsFeatLane<F> *)d_st, d_out, n, mode == FS_FEATURE_FIND, R, max_iters,
                                r->orbit_uncompressed, s);
        e = hipGetLastError();
    }
    // slices until no candidate is left running; each ends in a synchronisation (a launch lasts a fraction of a second)
    while (e == hipSuccess) {
        uint32_t left = 0;
        e = hipMemsetAsync(d_cnt, 0, sizeof(uint32_t), s);
        if (e != hipSuccess)
            break;
        const uint32_t slice = r->feature_slice ? r->feature_slice : kFeatureSlice;
        if (seq)
            fsk_feature_seq_step<F>(r->wp_raw, (uint32_t)r->orbit_size, c_low, r->orbit_uncompressed, d_st, d_out, n,
                                    mode == FS_FEATURE_FIND, iter_bytes == 8, slice, (uint32_t *)d_cnt, s);
        else
            fsk_feature_step<F>(zref, (uint32_t)r->orbit_uncompressed, (FsFeatLane<F> *)d_st, d_out, n, mode == FS_FEATURE_FIND,
                                iter_bytes == 8, slice, (uint32_t *)d_cnt, s);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(&left, d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (left == 0)
            break;
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(out, d_out, n * sizeof(Out), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    for (void *p : {d_in, d_out, d_st, d_cnt})
        if (p)
            (void)r_free(r, p);
    return (uint32_t)e;
}

// fs_feature_eval_direct: the same shape without an orbit (kernels_feature_direct.hip).
template <class F>
static uint32_t feature_eval_direct(fs_renderer *r, uint32_t iter_bytes, int mode, const void *radius, uint64_t max_iters,
                                    const void *in, void *out, uint64_t n)
{
    using In = typename FsFeatRec<F>::In;
    using Out = typename FsFeatRec<F>::Out;
    using Real = typename FsDev<F>::Real;
    const bool find = mode == FS_FEATURE_FIND;
    if (iter_bytes == 4 && !find)
        for (uint64_t k = 0; k < n; k++)
            if (((const In *)in)[k].period > 0xFFFFFFFFull)
                return hipErrorInvalidValue; // a period IterType cannot hold
    const Real rad = *(const Real *)radius;
    const fs::hreal<F> R{rad.m, rad.e};
    const uint32_t slice = r->feature_slice ? r->feature_slice : kFeatureSlice;
    hipStream_t s = r->compute;
    void *d_in = nullptr, *d_out = nullptr, *d_st = nullptr, *d_cnt = nullptr;
    hipError_t e = r_alloc(r, &d_in, n * sizeof(In), kFrame);
    if (e == hipSuccess)
        e = r_alloc(r, &d_out, n * sizeof(Out), kFrame);
    if (e == hipSuccess)
        e = r_alloc(r, &d_st, n * sizeof(FsFeatDirectLane<F>), kFrame);
    if (e == hipSuccess)
        e = r_alloc(r, &d_cnt, sizeof(uint32_t), kFrame);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_in, in, n * sizeof(In), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        fsk_feature_direct_init<F>(d_in, (FsFeatDirectLane<F> *)d_st, d_out, n, find, R, max_iters, s);
        e = hipGetLastError();
    }
    while (e == hipSuccess) {
        uint32_t left = 0;
        e = hipMemsetAsync(d_cnt, 0, sizeof(uint32_t), s);
        if (e != hipSuccess)
            break;
        fsk_feature_direct_step<F>((FsFeatDirectLane<F> *)d_st, d_out, n, find, iter_bytes == 8, R, slice, (uint32_t *)d_cnt, s);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(&left, d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (left == 0)
            break;
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(out, d_out, n * sizeof(Out), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    for (void *p : {d_in, d_out, d_st, d_cnt})
        if (p)
            (void)r_free(r, p);
    return (uint32_t)e;
}

// fs_feature_eval_plain / fs_feature_eval_plain_direct: the same shape for T = float / double (kernels_feature_plain.hip).
// form = kFeatPExpanded / kFeatPWaypoints / kFeatPDirect.
template <class T>
static uint32_t feature_eval_plain(fs_renderer *r, int form, uint32_t iter_bytes, int mode, const void *radius, uint64_t max_iters,
                                   const void *in, void *out, uint64_t n)
{
    using In = typename FsFeatPRec<T>::In;
    using Out = typename FsFeatPRec<T>::Out;
    const bool find = mode == FS_FEATURE_FIND;
    if (iter_bytes == 4 && !find)
        for (uint64_t k = 0; k < n; k++)
            if (((const In *)in)[k].period > 0xFFFFFFFFull)
                return hipErrorInvalidValue; // a period IterType cannot hold
    const T R = *(const T *)radius;
    const int u64 = iter_bytes == 8;
    const void *orbit = form == kFeatPWaypoints  ? (const void *)r->wp_raw
                        : form == kFeatPExpanded ? (sizeof(T) == 4 ? (const void *)r->orbit_plain : (const void *)r->orbit_f64)
                                                 : nullptr;
    const uint32_t n_wp = form == kFeatPWaypoints ? (uint32_t)r->orbit_size : 0u;
    const uint64_t count = form == kFeatPDirect ? 0 : r->orbit_uncompressed;
    T c_low[2] = {T(0), T(0)};
    if (form == kFeatPWaypoints) {
        memcpy(&c_low[0], r->c_low_plain[0], sizeof(T));
        memcpy(&c_low[1], r->c_low_plain[1], sizeof(T));
    }
    const uint32_t slice = r->feature_slice ? r->feature_slice : kFeatureSlice;
    hipStream_t s = r->compute;
    void *d_in = nullptr, *d_out = nullptr, *d_st = nullptr, *d_cnt = nullptr;
    hipError_t e = r_alloc(r, &d_in, n * sizeof(In), kFrame);
    if (e == hipSuccess)
        e = r_alloc(r, &d_out, n * sizeof(Out), kFrame);
    if (e == hipSuccess)
        e = r_alloc(r, &d_st, n * fsk_featp_lane_bytes<T>(form, u64), kFrame);
    if (e == hipSuccess)
        e = r_alloc(r, &d_cnt, sizeof(uint32_t), kFrame);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_in, in, n * sizeof(In), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        fsk_featp_init<T>(form, u64, d_in, d_st, d_out, n, find, R, max_iters, count, orbit, n_wp, s);
        e = hipGetLastError();
    }
    // slices until no candidate is left running; each ends in a synchronisation
    while (e == hipSuccess) {
        uint32_t left = 0;
        e = hipMemsetAsync(d_cnt, 0, sizeof(uint32_t), s);
        if (e != hipSuccess)
            break;
        fsk_featp_step<T>(form, u64, orbit, n_wp, c_low[0], c_low[1], count, d_st, d_out, n, find, R, slice, (uint32_t *)d_cnt, s);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(&left, d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (left == 0)
            break;
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(out, d_out, n * sizeof(Out), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    for (void *p : {d_in, d_out, d_st, d_cnt})
        if (p)
            (void)r_free(r, p);
    return (uint32_t)e;
}

extern "C" {

uint32_t fs_feature_eval_plain(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius, uint64_t max_iters,
                               const void *in, void *out, uint64_t n)
{
    if (uint32_t e = use_device(r))
        return e;
    if ((type_tag != FS_T_F32 && type_tag != FS_T_F64) || (iter_bytes != 4 && iter_bytes != 8) ||
        (mode != FS_FEATURE_FIND && mode != FS_FEATURE_FIXED))
        return FS_ERR_UNSUPPORTED;
    if (!r->compute || !r->orbit_ok || r->orbit_type != type_tag)
        return FS_ERR_6;
    const bool seq = r->orbit_seq;
    if (seq) {
        if (!r->wp_raw || r->orbit_size == 0)
            return FS_ERR_6;
        // positions are IterType-wide: 32-bit ones cannot walk an orbit of 2^32 entries and more
        if (iter_bytes == 4 && r->orbit_uncompressed > 0xFFFFFFFFull)
            return FS_ERR_UNSUPPORTED;
    } else if ((type_tag == FS_T_F32 ? (const void *)r->orbit_plain : (const void *)r->orbit_f64) == nullptr) {
        return FS_ERR_6;
    }
    if (n == 0)
        return 0;
    if (!radius || !in || !out)
        return hipErrorInvalidValue;
    const int form = seq ? kFeatPWaypoints : kFeatPExpanded;
    return type_tag == FS_T_F32 ? feature_eval_plain<float>(r, form, iter_bytes, mode, radius, max_iters, in, out, n)
                                : feature_eval_plain<double>(r, form, iter_bytes, mode, radius, max_iters, in, out, n);
}

uint32_t fs_feature_eval_plain_direct(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius,
                                      uint64_t max_iters, const void *in, void *out, uint64_t n)
{
    if (uint32_t e = use_device(r))
        return e;
    if ((type_tag != FS_T_F32 && type_tag != FS_T_F64) || (iter_bytes != 4 && iter_bytes != 8) ||
        (mode != FS_FEATURE_FIND && mode != FS_FEATURE_FIXED))
        return FS_ERR_UNSUPPORTED;
    if (n == 0)
        return 0;
    if (!radius || !in || !out)
        return hipErrorInvalidValue;
    if (uint32_t e = ensure_streams(r)) // no fs_init_memory needed
        return e;
    return type_tag == FS_T_F32 ? feature_eval_plain<float>(r, kFeatPDirect, iter_bytes, mode, radius, max_iters, in, out, n)
                                : feature_eval_plain<double>(r, kFeatPDirect, iter_bytes, mode, radius, max_iters, in, out, n);
}

uint32_t fs_feature_eval(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius, uint64_t max_iters,
                         const void *in, void *out, uint64_t n)
{
    if (uint32_t e = use_device(r))
        return e;
    if ((type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64) || (iter_bytes != 4 && iter_bytes != 8) ||
        (mode != FS_FEATURE_FIND && mode != FS_FEATURE_FIXED))
        return FS_ERR_UNSUPPORTED;
    if (!r->compute || !r->orbit_ok || r->orbit_type != type_tag)
        return FS_ERR_6;
    if (r->orbit_seq)
        return FS_ERR_UNSUPPORTED; // only the waypoints are resident: the evaluator reads the expanded orbit
    if ((type_tag == FS_T_HDR32 ? (const void *)r->zref : (const void *)r->zref64) == nullptr)
        return FS_ERR_6;
    if (n == 0)
        return 0;
    if (!radius || !in || !out)
        return hipErrorInvalidValue;
    return type_tag == FS_T_HDR32 ? feature_eval<float>(r, iter_bytes, mode, radius, max_iters, in, out, n)
                                  : feature_eval<double>(r, iter_bytes, mode, radius, max_iters, in, out, n);
}

int fs_orbit_form(const fs_renderer *r)
{
    return !r || !r->orbit_ok ? 0 : r->orbit_seq ? 2 : 1;
}

uint32_t fs_feature_eval_resident(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius,
                                  uint64_t max_iters, const void *in, void *out, uint64_t n)
{
    if (uint32_t e = use_device(r))
        return e;
    if ((type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64) || (iter_bytes != 4 && iter_bytes != 8) ||
        (mode != FS_FEATURE_FIND && mode != FS_FEATURE_FIXED))
        return FS_ERR_UNSUPPORTED;
    if (!r->compute || !r->orbit_ok || r->orbit_type != type_tag)
        return FS_ERR_6;
    const bool seq = r->orbit_seq;
    if (seq) {
        if (!r->wp_raw || r->orbit_size == 0)
            return FS_ERR_6;
        // positions are IterType-wide: 32-bit ones cannot walk an orbit of 2^32 entries and more
        if (iter_bytes == 4 && r->orbit_uncompressed > 0xFFFFFFFFull)
            return FS_ERR_UNSUPPORTED;
    } else if ((type_tag == FS_T_HDR32 ? (const void *)r->zref : (const void *)r->zref64) == nullptr) {
        return FS_ERR_6;
    }
    if (n == 0)
        return 0;
    if (!radius || !in || !out)
        return hipErrorInvalidValue;
    return type_tag == FS_T_HDR32 ? feature_eval<float>(r, iter_bytes, mode, radius, max_iters, in, out, n, seq)
                                  : feature_eval<double>(r, iter_bytes, mode, radius, max_iters, in, out, n, seq);
}

uint32_t fs_feature_eval_direct(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius, uint64_t max_iters,
                                const void *in, void *out, uint64_t n)
{
    if (uint32_t e = use_device(r))
        return e;
    if ((type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64) || (iter_bytes != 4 && iter_bytes != 8) ||
        (mode != FS_FEATURE_FIND && mode != FS_FEATURE_FIXED))
        return FS_ERR_UNSUPPORTED;
    if (n == 0)
        return 0;
    if (!radius || !in || !out)
        return hipErrorInvalidValue;
    if (uint32_t e = ensure_streams(r)) // no fs_init_memory needed
        return e;
    return type_tag == FS_T_HDR32 ? feature_eval_direct<float>(r, iter_bytes, mode, radius, max_iters, in, out, n)
                                  : feature_eval_direct<double>(r, iter_bytes, mode, radius, max_iters, in, out, n);
}

uint32_t fs_set_feature_slice(fs_renderer *r, uint32_t steps)
{
    if (!r)
        return hipErrorInvalidValue;
    r->feature_slice = steps;
    return 0;
}

// ---- fs_autozoom_pick: the host side.  One device block per call: [FsAzStats | Default's slab or FilamentTip's per-row counts |
// FilamentTip's gather buffer]; the kernels run back to back on the compute stream and hand their integers to one another
// through the block, the host reads it once they are through.
static constexpr uint32_t kAzGatherRows = 32; // frame rows the gather buffer holds by default (W records each)

uint32_t fs_set_autozoom_gather_cap(fs_renderer *r, uint32_t rows)
{
    if (!r)
        return hipErrorInvalidValue;
    r->az_gather_rows = rows;
    return 0;
}

uint32_t fs_autozoom_pick(fs_renderer *r, int heuristic, uint64_t n_iterations, const void *device_iters, fs_autozoom_result *out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!out)
        return hipErrorInvalidValue;
    if (heuristic != FS_AUTOZOOM_DEFAULT && heuristic != FS_AUTOZOOM_MAX && heuristic != FS_AUTOZOOM_FILAMENT_TIP)
        return FS_ERR_UNSUPPORTED;
    if (!r->memory_initialized() || !r->compute)
        return FS_ERR_6;
    if (r->local_rows != r->height)
        return FS_ERR_UNSUPPORTED; // this renderer holds some rows of the frame only
    const uint32_t W = r->width, H = r->height;
    const bool tip = heuristic == FS_AUTOZOOM_FILAMENT_TIP;
    constexpr uint32_t kMargin = 18; // AutoZoomer.cpp:250
    if (tip && (W <= 2 * kMargin || H <= 2 * kMargin))
        return FS_ERR_UNSUPPORTED;
    // Default's inner rectangle (AutoZoomer.cpp:78-93): an eighth of the SCREEN off each side, then scaled by the antialiasing
    uint32_t x0 = 0, y0 = 0, rw = W, rh = H;
    if (heuristic == FS_AUTOZOOM_DEFAULT) {
        const uint32_t sw = W / r->aa, sh = H / r->aa;
        x0 = sw / 8 * r->aa, y0 = sh / 8 * r->aa;
        rw = (sw - sw / 8) * r->aa - x0, rh = (sh - sh / 8) * r->aa - y0;
        if (!rw || !rh)
            return FS_ERR_UNSUPPORTED;
    }
    FsAzFrame F{device_iters ? device_iters : r->iters(), r->iter_bytes == 8 ? 1u : 0u, r->w_block * 16u, W, H, n_iterations};
    const uint32_t cap_rows = r->az_gather_rows ? r->az_gather_rows : kAzGatherRows;
    const uint64_t cap64 = (uint64_t)cap_rows * W;
    const uint32_t cap = tip ? (uint32_t)(cap64 < 0xFFFFFFFFull ? cap64 : 0xFFFFFFFFull) : 0;
    const size_t st_bytes = (sizeof(FsAzStats) + 255) / 256 * 256;
    const size_t mid_bytes = ((heuristic == FS_AUTOZOOM_DEFAULT ? (size_t)rh * 3 * sizeof(double) : tip ? (size_t)H * 4 : 0) + 255) / 256 * 256;
    void *blk = nullptr;
    hipStream_t s = r->compute;
    FS_TRY(r_alloc(r, &blk, st_bytes + mid_bytes + (size_t)cap * sizeof(FsAzTipRec), kFrame));
    FsAzStats *d_st = (FsAzStats *)blk;
    void *d_mid = (char *)blk + st_bytes;
    FsAzTipRec *d_rec = (FsAzTipRec *)((char *)blk + st_bytes + mid_bytes);
    // sqrt(double(W * W + H * H)) / 2.0 (AutoZoomer.cpp:357-358)
    const double max_dist = sqrt((double)((int64_t)W * W + (int64_t)H * H)) / 2.0;

    FsAzStats st{};
    std::vector<FsAzTipRec> recs;
    std::vector<uint32_t> row_counts;
    memset(out, 0, sizeof(*out));
    out->heuristic = (uint32_t)heuristic;
    // FilamentTip's decision among the gathered candidates: libm, raster order, strict `>` (AutoZoomer.cpp:252-254, 363-367)
    double best = -1.0;
    uint32_t best_x = W / 2, best_y = H / 2;
    uint64_t rescored = 0;
    auto rescore = [&](double avg) {
        std::sort(recs.begin(), recs.end(), [](const FsAzTipRec &a, const FsAzTipRec &b) { return a.y != b.y ? a.y < b.y : a.x < b.x; });
        for (const FsAzTipRec &c : recs) {
            const double sc = fs::az_tip_score(c.iter, c.high, c.x, c.y, W, H, n_iterations, avg, max_dist);
            rescored++;
            if (sc > best)
                best = sc, best_x = c.x, best_y = c.y;
        }
    };
    auto fetch = [&](uint64_t n) -> hipError_t { // the first n gathered records
        recs.resize(n);
        if (!n)
            return hipSuccess;
        const hipError_t e = hipMemcpyAsync(recs.data(), d_rec, n * sizeof(FsAzTipRec), hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    };

    r->az_seed = FsAzStats{};
    r->az_seed.first_index = ~0ull;
    hipError_t e = hipMemcpyAsync(d_st, &r->az_seed, sizeof(FsAzStats), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && tip)
        e = hipMemsetAsync(d_mid, 0, (size_t)H * 4, s);
    if (e == hipSuccess) {
        fsk_az_stats(F, x0, y0, rw, rh, d_st, s);
        if (heuristic == FS_AUTOZOOM_MAX) {
            fsk_az_max(F, d_st, s);
        } else if (heuristic == FS_AUTOZOOM_DEFAULT) {
            const double wo2 = (double)(int32_t)rw / 2.0, ho2 = (double)(int32_t)rh / 2.0;
            fsk_az_default(F, x0, y0, rw, rh, wo2, ho2, sqrt(wo2 * wo2 + ho2 * ho2), d_st, (double *)d_mid, s);
        } else {
            fsk_az_tip_score(F, max_dist, d_st, s);
            fsk_az_tip_gather(F, max_dist, kMargin, H - kMargin, d_st, d_rec, cap, (uint32_t *)d_mid, s);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(&st, d_st, sizeof(FsAzStats), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    const uint64_t n_rect = (uint64_t)rw * rh;
    const double avg = (double)st.sum / (heuristic == FS_AUTOZOOM_DEFAULT ? (double)(int32_t)(rh * rw) : (double)n_rect);
    if (e == hipSuccess && tip && st.gathered <= cap) {
        e = fetch(st.gathered);
        if (e == hipSuccess)
            rescore(avg);
    } else if (e == hipSuccess && tip) {
        // more qualify than the buffer holds (exact ties: a lattice, a symmetric frame): again over bands of consecutive rows that
        // fit, by the per-row counts the first launch recorded.  One row fits by construction (cap >= W).  Bands go top to bottom
        // and `best` is carried across them, so the decision is the raster-order one.
        row_counts.resize(H);
        e = hipMemcpyAsync(row_counts.data(), d_mid, (size_t)H * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        for (uint32_t ya = kMargin; e == hipSuccess && ya < H - kMargin;) {
            uint64_t n = 0;
            uint32_t yb = ya;
            while (yb < H - kMargin && n + row_counts[yb] <= cap)
                n += row_counts[yb++];
            if (yb == ya) { // (cannot happen: a row holds fewer than W candidates)
                e = hipErrorUnknown;
                break;
            }
            if (n) {
                e = hipMemsetAsync(&d_st->gathered, 0, sizeof(uint64_t), s);
                if (e == hipSuccess) {
                    fsk_az_tip_gather(F, max_dist, ya, yb, d_st, d_rec, cap, nullptr, s);
                    e = hipGetLastError();
                }
                if (e == hipSuccess)
                    e = fetch(n);
                if (e == hipSuccess)
                    rescore(avg);
            }
            ya = yb;
        }
    }
    (void)r_free(r, blk);
    if (e != hipSuccess)
        return (uint32_t)e;

    out->max_iter = st.max_iter;
    out->sum_iters = st.sum;
    out->avg = avg;
    if (heuristic == FS_AUTOZOOM_MAX) {
        out->num_at_limit = st.num_at_limit;
        out->num_at_max = st.n_ge;
        out->target_x = (double)(st.first_index % W);
        out->target_y = (double)(st.first_index / W);
        out->status = st.num_at_limit == n_rect ? FS_AUTOZOOM_FLAT : st.n_ge > 500 ? FS_AUTOZOOM_MOVE_THEN_STOP : FS_AUTOZOOM_MOVE;
    } else if (heuristic == FS_AUTOZOOM_DEFAULT) {
        out->num_at_limit = st.num_at_limit;
        out->num_at_max = st.num_at_max;
        out->sum_sq = st.sums[0], out->sum_sq_x = st.sums[1], out->sum_sq_y = st.sums[2];
        if (st.sums[0] == 0) {
            out->status = FS_AUTOZOOM_FLAT;
        } else {
            out->target_x = st.sums[1] / st.sums[0];
            out->target_y = st.sums[2] / st.sums[0];
            out->status = st.num_at_limit == n_rect      ? FS_AUTOZOOM_FLAT
                          : st.num_at_max > 500 ? FS_AUTOZOOM_MOVE_THEN_STOP
                                                : FS_AUTOZOOM_MOVE;
        }
    } else {
        out->num_at_max = st.num_at_max;
        out->candidates = st.candidates;
        out->accepted = st.accepted;
        out->run_reject = st.run_reject;
        for (int k = 0; k < 9; k++)
            out->high_hist[k] = st.hist[k];
        out->rescored = rescored;
        out->score = best;
        out->target_x = (double)best_x, out->target_y = (double)best_y;
        out->status = st.sum == 0 || best < 0 ? FS_AUTOZOOM_NO_TARGET : st.num_at_max > n_rect / 2 ? FS_AUTOZOOM_FLAT : FS_AUTOZOOM_MOVE;
    }
    return 0;
}

} // extern "C"
