/* fsmi355_internal.h -- measurement hooks, A/B switches and test read-backs of libfsmi355.so.
 *
 * NOT part of the drop-in boundary: nothing here replaces a GPURenderer member and a FractalShark maintainer never calls any of it
 * (include/fsmi355.h is the interface to bind).  bench.py, tests/ and tools/ use these entry points to time kernels, count executed
 * work, select the in-library A/B variants the defaults were measured against, and read device-built tables back for comparison
 * with the host builders.
 */
#ifndef FSMI355_INTERNAL_H
#define FSMI355_INTERNAL_H

#include "fsmi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Measurement hooks (this project's addition; bench.py / profiles).
 * fs_last_kernel_ms: duration of the most recent iteration-kernel launch measured with HIP events on the
 * compute stream (valid after fs_sync_compute).
 * fs_enable_step_count: when on, iteration kernels also accumulate the executed work per launch:
 * counts[0] = AT iterations, [1] = LA steps, [2] = perturbation steps, [3] = pixels,
 * [4] = lane slots occupied in the perturbation loop (64 x longest lane, summed over waves),
 * [5] = perturbation steps that went through the careful (exit-tested) path of the tuned LAv2 loop, [6] = steps taken in
 * its scaled runs, [7] = scaled runs started (both per lane). */
float fs_last_kernel_ms(const fs_renderer *r);
/* The durations of the last n (<= 64) iteration-kernel launches, oldest first (each launch keeps its own pair of HIP
 * events, so frames that were in flight together can be read after the fact); valid after fs_sync_compute. */
uint32_t fs_kernel_ms_history(const fs_renderer *r, float *ms_out, uint32_t n);
/* The same launches split where a frame is made of TWO kernels (HDRFloat<double> LAv2: k_at_pass64, then k_lav2_lit<double>):
 * first_ms[k] = the first kernel (0 for a one-kernel frame), second_ms[k] = the rest; first + second = fs_kernel_ms_history. */
uint32_t fs_kernel_ms_split_history(const fs_renderer *r, float *first_ms, float *second_ms, uint32_t n);
/* Low byte: 0 (default) = tuned iteration loops; 1 = literal operation-by-operation transcription of the CPU function;
 * 2 = tuned loops without the scaled runs of the HDRFloat<float> LAv2 kernel (slower; kept as in-library A/B references
 * for the tuned loops -- results are identical).  ORed with A/B flags, both off by default because they measure slower
 * (DESIGN.md 4.3 / 5.2), both bit-identical to the default and under test (tests/test_gpu_variants.py):
 *   FS_VARIANT_LDS_ORBIT  the scaled runs of the tuned HDRFloat<float> LAv2 kernel take their orbit entries through LDS
 *                         (LDS-DMA double buffer per wave) instead of the scalar cache;
 *   FS_VARIANT_REFILL     the HDRFloat<float|double> BLA kernel runs as a persistent launch whose waves refill finished
 *                         lanes from a frame-wide pixel queue (wave-ballot compaction).
 * Unknown values: hipErrorInvalidValue, the selection stays as it was.
 *   FS_VARIANT_WIDE_COUNTERS  (test switch) every entry point launches the instantiation of its kernel that counts
 *                         iterations in 64 bits -- the ones an iteration cap of 2^32 or above selects -- whatever the cap is:
 *                         lets the 64-bit kernels be compared with the CPU functions at caps a test can afford.
 *   FS_VARIANT_NATURAL_TILE_ORDER  fs_render_bla without BLA (perturbation only, HDRFloat<float>) and the tuned
 *                         HDRFloat<float> fs_render_lav2 (self-recorded order, see fs_forget_tile_costs) launch a frame's 8 x 8
 *                         tiles in their natural order.  Default for frames with an iteration limit of 2^18 or more and
 *                         at least 4096 tiles: the tiles that hold long-running pixels first (a probe launch runs every
 *                         tile's centre pixel for n_iterations / 32 steps), ONE to a workgroup with three
 *                         short tiles beside it (never-escaping waves that share a CU slow each other down) --
 *                         which wave renders which tile changes no pixel.
 *                         The same switch keeps the HDRFloat<double> / HDRFloat<CudaDblflt> fs_render_lav2 frames in the tile
 *                         mapping: by default, from the third frame of a view on (the first runs as it is, the second records and
 *                         sorts -- a view that is shown once pays for no sort; a view = same geometry, row bands, orbit, coordinates,
 *                         iteration limit, mode), lane s of the launch renders the pixel that ranked s-th in the previous
 *                         frame -- by iteration count (HDRFloat<double>) or by the cost that frame recorded per pixel, its own AT
 *                         iterations above its perturbation steps (HDRFloat<CudaDblflt>); a device radix sort, once per view;
 *                         frames of 2^20 elements and more -- so that the lanes of a wave run equally long.  Which lane renders
 *                         which pixel changes no pixel.
 *   FS_VARIANT_BLA_POOL   the hand-written HDRFloat<float> BLA kernel (the default of fs_render_bla with a table) re-packs the
 *                         running pixels of a workgroup's four waves into as few waves as possible every 32 trips (LDS exchange).
 *                         A/B, off by default: measured slower; results identical.
 */
enum { FS_VARIANT_LDS_ORBIT = 0x100, FS_VARIANT_REFILL = 0x200, FS_VARIANT_WIDE_COUNTERS = 0x400,
       FS_VARIANT_NATURAL_TILE_ORDER = 0x800, FS_VARIANT_BLA_POOL = 0x1000 };
uint32_t fs_set_kernel_variant(fs_renderer *r, int variant);
/* Longest tiles first, self-recorded (this project's addition).  Every fs_render_lav2 frame of the tuned
 * HDRFloat<float> kernel records one cost word per 8 x 8 tile (its longest lane's step count); the next frame with the
 * same geometry, row bands and orbit generation is launched in descending cost order -- "warm".  The first frame, a frame
 * after any of those changed or after fs_forget_tile_costs, and every frame under FS_VARIANT_NATURAL_TILE_ORDER run in
 * natural order -- "cold".  The order changes which wave renders which tile, never a pixel.
 * fs_render_bla's probe order (FS_VARIANT_NATURAL_TILE_ORDER above) is kept the same way: a frame with the same geometry, row
 * bands, orbit (generation, or for generation 0 a sampled fingerprint of the entries -- RenderPerturbBLA re-uploads per call),
 * coordinates and iteration limit as the one before reuses the order and skips the probe launch; fs_forget_tile_costs drops it
 * -- and the pixel order of the HDRFloat<double> / HDRFloat<CudaDblflt> LAv2 frames (FS_VARIANT_NATURAL_TILE_ORDER above).
 * fs_last_frame_tile_ordered: 1 when the most recent fs_render_lav2 launch used a recorded order / the most recent
 * perturbation-only fs_render_bla launch reused its probe order.
 * fs_last_frame_sampled_tile_order (round 6): 1 when the most recent fs_render_lav2 launch was a view's FIRST frame of the
 * HDRFloat<double> / HDRFloat<CudaDblflt> kernels with its tiles in the order of a sampled PerformAT count
 * (csrc/kernels_tile_sample.hip; A/B switch: environment FSMI355_COLD_TILE_ORDER=0, FS_VARIANT_NATURAL_TILE_ORDER).
 * fs_read_tile_costs: the costs the last frame recorded (row-major tiles of the LOCAL buffer, (width + 7) / 8 per row);
 * *n_tiles = their number; out may be NULL.  FractalSharkError 10006 when nothing has been recorded. */
uint32_t fs_forget_tile_costs(fs_renderer *r);
int fs_last_frame_tile_ordered(fs_renderer *r);
int fs_last_frame_sampled_tile_order(fs_renderer *r);
uint32_t fs_read_tile_costs(fs_renderer *r, uint32_t *out, uint64_t max_words, uint64_t *n_tiles);
/* Test hook for the waypoint-resident orbit (fs_set_compressed_orbit_mode(1), HDRFloat<float | double>): one lane's
 * decompression cursor -- with 32-bit positions, or the 64-bit ones the wide kernel uses -- seeks to orbit index `start`
 * and walks n entries on; out[k] = the orbit value at start + k as {float re, im; int32 e} (12 B) or
 * {double re, im; int32 e; pad} (24 B).  Indices of 2^32 and above need wide_positions = 1. */
uint32_t fs_seq_cursor_probe(fs_renderer *r, int wide_positions, uint64_t start, uint32_t n, void *out);
/* The launch order of the most recent frame when it was an ordered one (its first n_tiles words: a permutation of the tile
 * numbers, highest cost class first); 10006 otherwise.  For tests. */
uint32_t fs_read_tile_order(fs_renderer *r, uint32_t *out, uint64_t max_words);
/* Test hook: steps per candidate per launch of the Feature Finder evaluators (fs_feature_eval, fs_feature_eval_direct); 0 = the
 * default, 2^18.  A Direct period search never runs that long, so only a small slice exercises the lane state that is carried
 * from launch to launch.  Changes no result. */
uint32_t fs_set_feature_slice(fs_renderer *r, uint32_t steps);
/* Test hook: rows of the frame that the FilamentTip gather buffer of fs_autozoom_pick holds (W records each); 0 = the default,
 * 32.  When more candidates qualify than fit, the gather is repeated over bands of rows: a small cap exercises that path.
 * Changes no result. */
uint32_t fs_set_autozoom_gather_cap(fs_renderer *r, uint32_t rows);
/* Test and measurement hooks of the exact renderer (fs_render_exact, fs_exact_stable_mask).
 * fs_set_exact_slice: steps per sample per launch; 0 = the default: 4096, fewer while the list of running samples is long enough to
 * make such a launch last more than about 50 ms, never under 64.  A small slice makes a frame of hundreds of launches and
 * exercises the sample state that is carried from one to the next.  no_compaction = 1 (A/B): the running samples keep their slots
 * from slice to slice instead of being packed into full waves.  Neither changes a pixel.
 * fs_read_exact_stats: what the last call did, summed over its frames: out[0] = lane slots its waves occupied in the step loop
 * (64 x the steps of each wave's longest lane, per slice), [1] = steps its samples took, [2] = launches, [3] = samples still
 * running after each frame's first slice. */
uint32_t fs_set_exact_slice(fs_renderer *r, uint32_t steps, int no_compaction);
uint32_t fs_read_exact_stats(const fs_renderer *r, uint64_t out[4]);
/* The wide path (fs_exact_sample_counts, fs_render_exact_wide, fs_exact_eval_points_wide) obeys fs_set_exact_slice too (its default: about 50 ms of a lone
 * wave's steps at the limb count, divided by the number of times the list fills the chip's 1024 SIMDs, never under 16;
 * no_compaction is ignored: a launch has exactly one wave per running sample) and reports out[1] = steps its samples took (one
 * wave each, so out[0] = 64 x that), [2] = launches, [3] = samples still running after the first launch.
 * fs_exact_wide_state: the state of the wide kernel after `steps` steps from z_1 = c, every limb of it: out_x[l * n_samples + i],
 * out_y likewise (host memory, cx / cy as fs_exact_sample_counts).  No count stops a sample; the one thing that does is the bound
 * the limb count is derived from: a z with |z|^2 > 256 * 2^2F is kept as it is (its successors need not fit the limbs).  An escape
 * count is blind to wrong low limbs over a short run; the state shows a dropped carry at once.  Leaves fs_read_exact_stats alone. */
uint32_t fs_exact_wide_state(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                             uint32_t n_samples, uint32_t steps, uint32_t *out_x, uint32_t *out_y);
/* The cycle check of the exact renderer (fs_set_exact_cycle_check of fsmi355.h).
 * fs_read_exact_cycle_stats: of the last exact call, summed over its frames: out[0] = samples finished by proof, [1] = times a lane
 * read its checkpoint back for the full compare (fs_read_exact_stats reports what it reports without the check).
 * fs_set_exact_cycle_fingerprint_bits (test hook): a lane reads its checkpoint back only when a fingerprint matches: the low limbs
 * of x and y, 64 bits, so that the full compare runs next to never unless its answer is "equal".  bits = 1 .. 63 keeps that many low
 * bits of the 64-bit number (y[0] : x[0]) -- up to 32, bits of x[0] only -- and makes the compare run, and answer "not equal", on
 * one step in 2^bits; 0 = the default, all 64.  Changes no result. */
uint32_t fs_read_exact_cycle_stats(const fs_renderer *r, uint64_t out[2]);
uint32_t fs_set_exact_cycle_fingerprint_bits(fs_renderer *r, uint32_t bits);
/* The period planes of the exact renderer (fs_set_exact_periods of fsmi355.h).
 * fs_set_exact_atom_key_bits (test hook): a lane reads a pixel's smallest norm back only when the 64-bit key of the new norm equals
 * the key of the minimum.  bits = 6 .. 63 keeps that many top bits of the key (below 6: 6, the index of the highest limb that is not
 * zero alone) and makes the full compare run, and answer "not less", often; 0 = the default, all 64.  Changes no result. */
uint32_t fs_set_exact_atom_key_bits(fs_renderer *r, uint32_t bits);
uint32_t fs_enable_step_count(fs_renderer *r, int enable);
uint32_t fs_read_step_count(fs_renderer *r, uint64_t counts[8]);
/* The whole statistics buffer (measurement builds append per-wave trace records behind the 8 counters: library built
 * with FS_TRACE_WAVES=1 and FSMI355_TRACE_WAVES=<max waves> in the environment; tools/wave_trace.py). */
uint32_t fs_read_stats_raw(fs_renderer *r, uint64_t *out, uint64_t max_words);
/* Test hook: the wave-uniform block threshold of the tuned HDRFloat<float> LAv2 loop (csrc/kernels_lav2_hdr32.hip, FS_FAST_LOOP_FDU), evaluated on
 * the device by the macro the loop itself uses, for n triples (block bound as a binary32 bit pattern -- 0x80000000 = "never" --, largest
 * scale shift of the running lanes, largest max|dc| as a bit pattern): threshold_out[i] = -1 when dc_bits > bound_bits, else
 * min(bound_bits - scale_shift, 0x46800000) without wrap-around.  Host arrays.  tests/test_gpu_block_threshold.py. */
uint32_t fs_test_block_threshold(fs_renderer *r, const int32_t *bound_bits, const int32_t *scale_shift, const int32_t *dc_bits,
                                 int32_t *threshold_out, uint32_t n);
/* The same for the threshold of that loop's bodies without the dz add (NDZ; bound_bits = the NDZ body bound, taken for both of its terms): -1 when dc_bits >
 * bound_bits, else min(bound_bits - scale_shift, 0x3D000000) without wrap-around.  tests/test_gpu_lav2_ndz.py. */
uint32_t fs_test_ndz_threshold(fs_renderer *r, const int32_t *bound_bits, const int32_t *scale_shift, const int32_t *dc_bits,
                               int32_t *threshold_out, uint32_t n);
/* Read-back of what k_make_quiet_orbit made of the current HDRFloat<float> orbit for that loop (after fs_upload_orbit):
 * bounds_out[2 j], [2 j + 1] = the NDZ body bounds of entry j on max|dz| and on max|dc| (-0.0 = "never", both then), entries_out[4 j ..] = the second companion {2Z.re, 2Z.im, the entry's own bound, its
 * block bound} as the loop reads them; either may be NULL.  At most max_entries entries; *n_out = entries the orbit has (its two spare
 * entries included).  Synchronises the compute stream.  tests/test_gpu_lav2_ndz_tight.py holds the bounds against their definition. */
uint32_t fs_read_ndz_bounds(fs_renderer *r, float *bounds_out, float *entries_out, uint64_t max_entries, uint64_t *n_out);
/* Read-back of everything an orbit's upload leaves on the device for the tuned loops, part by part, as the kernels read it (m = the
 * orbit's entries + its two spare ones; tests/test_gpu_quiet_orbit.py holds every part against tests/_quiet_model.py bit for bit).
 * Of the current expanded HDRFloat<float> orbit: PREPARED = m float4 {re, im, exp, 2^(8 - 2 exp)}; FIRST = m float4 {re, im, ~exp + 116 or
 * the poison, 0}; SECOND = m float4 {2Z.re, 2Z.im, own bound, block bound}; ZS2 = (m + 32) float2, ZQB = (m + 32) float4 and ZNZ =
 * (m + 32) float2, the compact forms of the 16-step body and the NDZ body bounds, each with its 32 entries of slack.  Of the current expanded
 * HDRFloat<double> orbit: PREPARED64 = m FsZ64 {re, im, exp, 0, 2^(8 - 2 exp)} (32 B).  SCALED_F32: the binary32 entries of the last
 * fs_upload_orbit_scaled (fs_orbit_f32_bad; no spare entries) with the scaled kernels' bound word in `padding`.  *bytes = size of the
 * part; at most max_bytes are copied (out may be NULL).  FS_ERR_6: no such orbit is resident; FS_ERR_7: no such part.  Synchronises the
 * compute stream. */
enum { FS_QUIET_PART_PREPARED = 0, FS_QUIET_PART_FIRST = 1, FS_QUIET_PART_SECOND = 2, FS_QUIET_PART_ZS2 = 3, FS_QUIET_PART_ZQB = 4,
       FS_QUIET_PART_ZNZ = 5, FS_QUIET_PART_PREPARED64 = 6, FS_QUIET_PART_SCALED_F32 = 7 };
uint32_t fs_read_quiet_orbit(fs_renderer *r, int part, void *out, uint64_t max_bytes, uint64_t *bytes);
/* Average duration (HIP events on the compute stream, `repeats` back-to-back launches, no D2H) of the two RenderCurrent
 * kernels over the current iteration buffer: ms_out[0] = antialias + palette, ms_out[1] = min / max / sum.  Needs a
 * palette (fs_init_memory) and the whole frame on this renderer.  tools/bench_render_current.py turns them into GB/s. */
uint32_t fs_time_render_current(fs_renderer *r, uint64_t n_iterations, uint32_t repeats, float ms_out[2]);
/* Test read-back: the renderer's own colour buffer as it stands (fs_color_buffer_elements Color16) to the host, without running
 * the colour kernel first as fs_render_current does -- what an earlier call left in it (tests/current/torch_current.py:
 * fs_colorize_frame with device_colors leaves it alone).  Synchronises the compute stream. */
uint32_t fs_read_color_buffer(fs_renderer *r, fs_color16 *out);


/* ---- read-backs of device-built tables (tests, tools) */
/* Table geometry / contents after fs_build_bla or fs_upload_bla (tests, tools): number of levels (m_B.size()), m_LM2,
 * records per level; fs_read_bla_level copies one level to the host (synchronises the compute stream). */
int32_t fs_bla_num_levels(const fs_renderer *r);
int32_t fs_bla_lm2(const fs_renderer *r);
uint64_t fs_bla_level_size(const fs_renderer *r, int32_t level);
uint32_t fs_read_bla_level(fs_renderer *r, int32_t level, void *out, uint64_t max_records);
/* Test hook: BLAS::LookupBackwards as the device has it, asked directly.  which = 0: the lookup on the reference-layout levels in
 * HDRFloat<float> (HDRFloat<double> kernels, 64-bit counters, FS_VARIANT_LITERAL share its text), 1: the same in HDRFloat<double>,
 * 2: the lookup on the ladder and pre-test keys of the device-native form (the compiled kernel of variant 2; made first when stale,
 * which needs the HDRFloat<float> orbit).  Question i = (orbit index m[i], |dz|^2 = z2[i] as fs_real_hdr32, fs_real_hdr64 for
 * which = 1); level_ix_out[2 i], [2 i + 1] = level and element index of the record found, 0xFFFFFFFF twice for none.  Host arrays.
 * FS_ERR_6: no table of that type with more than two levels (no lookup can apply); FS_ERR_7: an m beyond the table. */
uint32_t fs_bla_lookup_probe(fs_renderer *r, int which, const uint32_t *m, const void *z2, uint32_t n, uint32_t *level_ix_out);
/* Read-back of the device-native forms of the HDRFloat<float> table (kernels.h: FsBlaRec, ladder, pre-test keys; kernels_bla_fast.hip:
 * heap records, heap ladder, Q, zb), made first when they are stale, as fs_render_bla does.  *bytes = size of the part; at most
 * max_bytes are copied (out may be NULL).  FS_BLA_PART_GEOMETRY: 16 + 2 x 40 uint32 -- [0] native form made, [1] heap form made,
 * [2] levels, [3] lm2, [4] native positions, [5] heap height H, [6] heap positions, [7] pre-test keys / Q entries, [8] orbit entries,
 * [16 + L] offset of level L, [56 + L] elements of level L.  FS_ERR_6: the part is not made (FS_BLA_PART_RECORDS .. PRETEST need
 * [0], the later parts [1]). */
enum { FS_BLA_PART_GEOMETRY = 0, FS_BLA_PART_RECORDS = 1, FS_BLA_PART_LADDER = 2, FS_BLA_PART_PRETEST = 3,
       FS_BLA_PART_HEAP_RECORDS = 4, FS_BLA_PART_HEAP_LADDER = 5, FS_BLA_PART_Q = 6, FS_BLA_PART_ZB = 7 };
uint32_t fs_read_bla_native(fs_renderer *r, int part, void *out, uint64_t max_bytes, uint64_t *bytes);
uint32_t fs_la_counts(const fs_renderer *r, uint32_t *n_las, uint32_t *n_stages, int *use_at, int *is_valid);
uint32_t fs_read_la(fs_renderer *r, void *las_out, uint32_t max_las, void *stages_out, uint32_t max_stages, void *at_out);

/* Duration of the last gather + reassembly on device 0 (HIP events; synchronises device 0's post stream). */
float fs_group_gather_ms(fs_group *g);

#ifdef __cplusplus
}
#endif

#endif /* FSMI355_INTERNAL_H */
