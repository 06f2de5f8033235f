// autozoom_ref.cpp -- the checker of fs_autozoom_pick: the AutoZoomer's three frame scans on ONE sequential thread over a host
// array, every sum in raster order, every score with libm.  It fills the record of include/fs_layout.h (fs_autozoom_result)
// the way that header says, with rescored = 0 (the checker scores every accepted candidate; the field counts what the
// library's host side scored).  Built by the tests with g++ -O2 -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/fs_layout.h"

namespace {

enum { kDefault = 0, kMax = 1, kTip = 2 };
enum { kMove = 0, kMoveThenStop = 1, kFlat = 2, kNoTarget = 3 };

template <class IterT> struct Frame {
    const IterT *p;
    uint32_t pitch;
    int W, H;
    uint64_t at(int x, int y) const { return p[(size_t)y * pitch + (size_t)x]; }
};

template <class IterT> void pick_max(const Frame<IterT> &f, uint64_t N, fs_autozoom_result *o)
{
    uint64_t top = 0;
    double total = 0; // exact below 2^53
    for (int y = 0; y < f.H; y++)
        for (int x = 0; x < f.W; x++) {
            const uint64_t v = f.at(x, y);
            total += (double)v;
            if (v > top)
                top = v;
        }
    bool found = false;
    uint64_t at_limit = 0, at_max = 0;
    for (int y = 0; y < f.H; y++)
        for (int x = 0; x < f.W; x++) {
            const uint64_t v = f.at(x, y);
            if (v == top) {
                at_limit++;
                if (!found) {
                    found = true;
                    o->target_x = x, o->target_y = y;
                }
            }
            if (v >= N)
                at_max++;
        }
    const uint64_t pixels = (uint64_t)f.W * (uint64_t)f.H;
    o->max_iter = top, o->num_at_limit = at_limit, o->num_at_max = at_max;
    o->sum_iters = (uint64_t)total, o->avg = total / (double)pixels;
    o->status = at_limit == pixels ? kFlat : at_max > 500 ? kMoveThenStop : kMove;
}

template <class IterT> void pick_default(const Frame<IterT> &f, int aa, uint64_t N, fs_autozoom_result *o)
{
    const int sw = f.W / aa, sh = f.H / aa;
    const int left = sw / 8 * aa, right = (sw - sw / 8) * aa, top_row = sh / 8 * aa, bottom = (sh - sh / 8) * aa;
    const int rw = right - left, rh = bottom - top_row;
    uint64_t top = 0;
    double total = 0;
    for (int y = top_row; y < bottom; y++)
        for (int x = left; x < right; x++) {
            const uint64_t v = f.at(x, y);
            total += (double)v;
            if (v > top)
                top = v;
        }
    const double avg = total / (double)(rh * rw);
    const double half_w = rw / 2.0, half_h = rh / 2.0;
    const double far = std::sqrt(half_w * half_w + half_h * half_h);
    double s = 0, sx = 0, sy = 0;
    uint64_t at_limit = 0, at_max = 0;
    for (int y = top_row; y < bottom; y++)
        for (int x = left; x < right; x++) {
            const uint64_t v = f.at(x, y);
            if (v == top)
                at_limit++;
            if ((double)v < avg)
                continue;
            // distance to the nearest edge of the rectangle along each axis: |h - |h - d||
            const double ex = std::fabs(half_w - std::fabs(half_w - std::fabs((double)(x - left))));
            const double ey = std::fabs(half_h - std::fabs(half_h - std::fabs((double)(y - top_row))));
            double weight = (double)v / (double)N;
            if (v == top)
                weight *= weight;
            const double edge = std::sqrt(ex * ex + ey * ey) / far;
            const double sq = weight * edge;
            s += sq;
            sx += sq * x;
            sy += sq * y;
            if (v >= N)
                at_max++;
        }
    o->max_iter = top, o->num_at_limit = at_limit, o->num_at_max = at_max;
    o->sum_iters = (uint64_t)total, o->avg = avg;
    o->sum_sq = s, o->sum_sq_x = sx, o->sum_sq_y = sy;
    if (s == 0) {
        o->status = kFlat;
        return;
    }
    o->target_x = sx / s, o->target_y = sy / s;
    o->status = at_limit == (uint64_t)rw * (uint64_t)rh ? kFlat : at_max > 500 ? kMoveThenStop : kMove;
}

template <class IterT> void pick_tip(const Frame<IterT> &f, uint64_t N, fs_autozoom_result *o)
{
    const int W = f.W, H = f.H;
    uint64_t top = 0;
    double total = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const uint64_t v = f.at(x, y);
            total += (double)v;
            if (v > top)
                top = v;
        }
    const uint64_t pixels = (uint64_t)W * (uint64_t)H;
    o->max_iter = top, o->sum_iters = (uint64_t)total;
    o->avg = pixels ? total / (double)pixels : 0;
    o->score = -1.0, o->target_x = W / 2, o->target_y = H / 2;
    o->status = kNoTarget;
    if (pixels == 0 || total == 0)
        return;
    const double avg = total / (double)pixels;
    const uint64_t threshold = (uint64_t)(avg + 1);
    // the ring of 8 directions, clockwise from "up"
    static const int ring_x[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    static const int ring_y[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
    const int margin = 18, radius = 12;
    double best = -1.0;
    int best_x = W / 2, best_y = H / 2;
    uint64_t at_max = 0;
    for (int y = margin; y < H - margin; y++)
        for (int x = margin; x < W - margin; x++) {
            const uint64_t v = f.at(x, y);
            if (v < threshold)
                continue;
            o->candidates++;
            if (v >= N)
                at_max++;
            const uint64_t floor_v = v > 0 ? v - 1 : v;
            bool high[8];
            int n_high = 0;
            for (int d = 0; d < 8; d++) {
                const int px = x + ring_x[d] * radius, py = y + ring_y[d] * radius;
                high[d] = px >= 0 && px < W && py >= 0 && py < H && f.at(px, py) >= floor_v;
                n_high += high[d] ? 1 : 0;
            }
            int longest = 0, run = 0;
            for (int i = 0; i < 16; i++) { // twice round the ring: runs that wrap
                run = high[i % 8] ? run + 1 : 0;
                if (run > longest)
                    longest = run;
            }
            o->high_hist[n_high]++;
            if (n_high > 3)
                continue;
            if (n_high > 0 && longest < n_high) {
                o->run_reject++;
                continue;
            }
            o->accepted++;
            const double tipness = 1.0 - (double)n_high / 4.0;
            const double above = (double)v - avg, span = (double)N - avg;
            const double raw = span > 0 ? std::log(1.0 + above) / std::log(1.0 + span) : 0.5;
            const double elevation = 1.0 - raw;
            const double cx = (double)(x - W / 2), cy = (double)(y - H / 2);
            const double far = std::sqrt((double)((int64_t)W * W + (int64_t)H * H)) / 2.0;
            const double off_centre = std::sqrt(cx * cx + cy * cy) / far;
            const double score = tipness * elevation * (0.3 + 0.7 * off_centre);
            if (score > best)
                best = score, best_x = x, best_y = y;
        }
    o->num_at_max = at_max;
    o->score = best, o->target_x = best_x, o->target_y = best_y;
    o->status = best < 0 ? kNoTarget : at_max > pixels / 2 ? kFlat : kMove;
}

template <class IterT>
int pick(int heuristic, const void *iters, uint32_t pitch, uint32_t W, uint32_t H, uint32_t aa, uint64_t N, fs_autozoom_result *o)
{
    const Frame<IterT> f{(const IterT *)iters, pitch, (int)W, (int)H};
    std::memset(o, 0, sizeof(*o));
    o->heuristic = (uint32_t)heuristic;
    if (heuristic == kMax)
        pick_max(f, N, o);
    else if (heuristic == kDefault)
        pick_default(f, (int)aa, N, o);
    else if (heuristic == kTip)
        pick_tip(f, N, o);
    else
        return 1;
    return 0;
}

} // namespace

// iters: H rows of `pitch` elements (uint32_t, or uint64_t when iter_u64), W x H valid (antialiasing included).  0 = done.
extern "C" int azr_pick(int heuristic, const void *iters, int iter_u64, uint32_t pitch, uint32_t W, uint32_t H, uint32_t aa,
                        uint64_t n_iterations, fs_autozoom_result *out)
{
    if (!iters || !out || !W || !H || !aa || W % aa || H % aa)
        return 1;
    return iter_u64 ? pick<uint64_t>(heuristic, iters, pitch, W, H, aa, n_iterations, out)
                    : pick<uint32_t>(heuristic, iters, pitch, W, H, aa, n_iterations, out);
}
