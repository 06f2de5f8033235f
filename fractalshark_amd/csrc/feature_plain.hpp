// feature_plain.hpp -- the Feature Finder's evaluators for the plain numeric types, T = float / double (kernels_feature_plain.hip;
// fs_feature_eval_plain, fs_feature_eval_plain_direct): one candidate's state between the bounded launches, and the launchers.
#pragma once
#include "kernels.h"

// The ABI records by type (include/fs_layout.h).
template <class T> struct FsFeatPRec;
template <> struct FsFeatPRec<float> {
    using In = fs_feature_in_f32;
    using Out = fs_feature_out_f32;
    using Orbit = fs_orbit_f32;
    using Waypoint = fs_orbit_f32_rc;
};
template <> struct FsFeatPRec<double> {
    using In = fs_feature_in_f64;
    using Out = fs_feature_out_f64;
    using Orbit = fs_orbit_f64;
    using Waypoint = fs_orbit_f64_rc;
};

template <class T> struct FsPC { // FloatComplex<T>
    T re, im;
};

// One PT candidate on the expanded orbit (phase: fsfeat::kPhasePT / kPhaseDirect / kPhaseDone, as FsFeatLane in kernels.h).
// PeriodicityPP's SqrNearLinearRadiusScale is the constant (0.25)^2 and is not kept.
template <class T> struct FsFeatPLane {
    FsPC<T> z, dz, dzdc, zcoeff, dc, c;
    T sqr_r; // PeriodicityPP::SqrNearLinearRadius
    uint64_t step, cap, period;
    uint32_t ref, phase;
};
// ... on a waypoint-resident orbit: positions as wide as the IterType (PosT), and the lane's decompression cursor -- the orbit
// value at `ref` (zx, zy), the number of the first waypoint behind it and that waypoint's orbit index.
template <class T, class PosT> struct FsFeatPSeqLane {
    FsPC<T> z, dz, dzdc, zcoeff, dc, c;
    T sqr_r;
    T zx, zy;
    uint64_t step, cap, period;
    PosT ref, next_index;
    uint32_t next, phase;
};
// The Direct evaluator's candidate (phase: kPhaseFindDirect / kPhaseDirect / kPhaseDone).
template <class T> struct FsFeatPDirectLane {
    FsPC<T> z, dzdc, zcoeff, c;
    uint64_t step, cap, period;
    uint32_t phase, pad_;
};

// form: how the candidates meet the orbit.
enum { kFeatPExpanded = 0, kFeatPWaypoints = 1, kFeatPDirect = 2 };

// Bytes of one candidate's state.
template <class T> size_t fsk_featp_lane_bytes(int form, int iter_u64);
// Set up n candidates from their fs_feature_in_f32 / _f64 records (wp / n_wp: the waypoints, kFeatPWaypoints only; count: the
// orbit's uncompressed length, unused by kFeatPDirect).
template <class T>
void fsk_featp_init(int form, int iter_u64, const void *in, void *st, void *out, uint64_t n, int find, T R, uint64_t max_iters,
                    uint64_t count, const void *wp, uint32_t n_wp, hipStream_t s);
// Advance every unfinished candidate by at most `slice` steps; *unfinished (zeroed by the caller) counts those still running
// afterwards.  orbit = the expanded fs_orbit_f32 / fs_orbit_f64 array (kFeatPExpanded) or the waypoints (kFeatPWaypoints, with
// n_wp and the decompressor's constant cx + i cy); R: kFeatPDirect only.
template <class T>
void fsk_featp_step(int form, int iter_u64, const void *orbit, uint32_t n_wp, T cx, T cy, uint64_t count, void *st, void *out,
                    uint64_t n, int find, T R, uint32_t slice, uint32_t *unfinished, hipStream_t s);
