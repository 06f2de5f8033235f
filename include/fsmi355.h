/* fsmi355.h -- C ABI of libfsmi355.so, the MI355X (gfx950) per-pixel renderer for FractalShark.
 *
 * One opaque fs_renderer corresponds to one reference `GPURenderer` object
 * (FractalSharkLib/GPU_Render.h:20-227, implemented by FractalSharkGpuLib/GPU_Render.cu).  Every entry
 * point below names the GPURenderer member it replaces; fractalshark_amd/csrc/gpu_render_shim.hpp defines
 * those members (same names, argument order and error behaviour) by forwarding here, so Fractal.cpp keeps
 * compiling against GPU_Render.h unchanged.  INTEGRATION.md shows the binding.
 *
 * Conventions (same as the reference):
 *   - every call returns uint32_t; 0 = success; non-zero = hipError_t value or FS_ERR_* (10000+);
 *   - host pointers are borrowed for the duration of the call only; device memory is owned by the renderer;
 *   - one renderer is used by one host thread at a time; different renderers may run concurrently;
 *   - "memory not initialised" makes render calls return 0 without doing anything (GPU_Render.cu:564-566).
 *
 * Record layouts: fs_layout.h.  Type tags select the numeric type T of the reference templates.
 *
 * This header is the whole interface a FractalShark maintainer binds: what gpu_render_shim.hpp forwards to, the device-side
 * table builders, and the multi-GPU group.  Measurement hooks, A/B switches and test read-backs the library also exports
 * (bench.py, tests/, tools/) are declared in fsmi355_internal.h and are not part of the drop-in boundary.
 */
#ifndef FSMI355_H
#define FSMI355_H

#include <stddef.h>
#include <stdint.h>

#include "fs_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fs_renderer fs_renderer;

/* FractalSharkError, GPU_Render.cu:33-43 (enum starts at 10000). */
enum {
    FS_OK = 0,
    FS_ERR_1 = 10000,
    FS_ERR_2 = 10001,
    FS_ERR_3 = 10002, /* bad antialiasing */
    FS_ERR_4 = 10003, /* width not divisible by antialiasing */
    FS_ERR_5 = 10004, /* height not divisible by antialiasing */
    FS_ERR_6 = 10005, /* no uploaded orbit / table for this type */
    FS_ERR_7 = 10006,
    FS_ERR_UNSUPPORTED = 10100 /* type tag / mode not built into this library (this project's addition) */
};

/* Numeric type T of the reference's kernel templates. */
enum {
    FS_T_F32 = 0,       /* float                      (Gpu1x32*)   */
    FS_T_F64 = 1,       /* double                     (Gpu1x64*)   */
    FS_T_2X32 = 2,      /* CudaDblflt<dblflt>         (Gpu2x32*)   */
    FS_T_HDR32 = 3,     /* HDRFloat<float>            (GpuHDRx32*) */
    FS_T_HDR64 = 4,     /* HDRFloat<double>           (GpuHDRx64*) */
    FS_T_HDR2X32 = 5,   /* HDRFloat<CudaDblflt<..>>   (GpuHDRx2x32*) */
    FS_T_2X64 = 6,      /* MattDbldbl (double-double) (Gpu2x64)      */
    FS_T_4X32 = 7,      /* MattQFltflt (quad-float)   (Gpu4x32)      */
    FS_T_4X64 = 8       /* MattQDbldbl (quad-double)  (Gpu4x64)      */
};

/* LAv2Mode, FractalSharkLib/RenderAlgorithm.h:12-17. */
enum { FS_LAV2_FULL = 0, FS_LAV2_PO = 1, FS_LAV2_LAO = 2 };

/* Which arithmetic the kernels restate.  The reference's CUDA kernels and its CPU RenderAlgorithm functions
 * are not bit-identical to each other; the parity target of this project is the CPU
 * functions, so FS_PARITY_CPU is the default everywhere.
 *   FS_PARITY_CPU      : literal CPU functions, including LAReference::isLAStageInvalid as written
 *                        (LAReference.cpp:1076-1081: stage skipped when cheb(dc) <  LAThresholdC).
 *   FS_PARITY_CPU_GPUSTAGE : CPU arithmetic, but the stage-validity test in the direction the reference's GPU
 *                        twin (and FractalZoomer) uses (GPU_LAReference.h:240-254: skipped when cheb(dc) >= ...).
 */
enum { FS_PARITY_CPU = 0, FS_PARITY_CPU_GPUSTAGE = 1 };

/* GPURenderer::GPURenderer / ~GPURenderer.  `device` = HIP device ordinal (the reference hard-codes 0,
 * GPU_Render.cu:113; the multi-GPU row tiler passes LOCAL_RANK). */
fs_renderer *fs_create(int device);
void fs_destroy(fs_renderer *r);

/* GPURenderer::TestCudaIsWorking (GPU_Render.cu:100-123): NON-ZERO = a usable device exists. */
uint32_t fs_test_device_is_working(void);

/* Number of HIP devices this process can see (0 when there is none or the runtime fails): what a multi-GPU host sizes
 * fs_group_create with.  This project's addition (the reference is single-device). */
int fs_device_count(void);

/* GPURenderer::ConvertErrorToString (GPU_Render.cu:1820-1823). */
const char *fs_error_string(uint32_t err);

/* GPURenderer::InitializeMemory<IterType> (GPU_Render.cu:232-407).  w,h already include antialiasing.
 * iter_bytes = sizeof(IterType) (4 or 8).  The iteration buffer is padded to 16 columns x 8 rows
 * (GPU_Render.cu:334-344).
 * IterType = uint64_t: the iteration buffer, RenderCurrent and ReductionResults work on uint64_t elements and the
 * uint64_t record layouts (fs_la_*_u64, fs_la_stage_u64, fs_at_*_u64) are accepted (table step lengths / indices must
 * fit 32 bits -- a table that large would not fit any device -- else FS_ERR_UNSUPPORTED).  Iteration caps of 2^32 and
 * above are served by every render entry point and numeric type: each kernel is also instantiated with 64-bit counters, as
 * the reference's kernels are templated on IterType (GPU_Render.cu:849-991, 1204-1300, 1380-1436, 1610-1692) -- for the
 * HDRFloat<float> perturbation kernels the literal form (the tuned runs budget their steps in 32 bits).  Such a cap with a
 * 4-byte buffer is a caller error (hipErrorInvalidValue): a uint32_t IterType cannot hold the count (every built-in view
 * selects Bits32, FractalViewPresets.cpp:19). */
uint32_t fs_init_memory(fs_renderer *r, uint32_t w, uint32_t h, uint32_t antialiasing, uint32_t iter_bytes,
                        const fs_color16 *pal_interleaved, uint32_t pal_iters, uint32_t palette_aux_depth,
                        uint64_t palette_generation, int expected_reuse);

/* Row band for multi-GPU tiling (this project's addition; the reference is single-device).  The renderer
 * keeps the full-frame geometry for the pixel -> delta-c mapping (Y stays the global row so
 * DeltaImaginary = -dy*T(Y) - centerY rounds identically) but only computes global rows
 * [band_first_row + k*band_stride_rows, +band_rows) for k = 0,1,...  The local iteration buffer then holds
 * the owned bands back to back.  Defaults: first 0, rows = h, stride = h (whole frame). */
uint32_t fs_set_row_bands(fs_renderer *r, uint32_t band_first_row, uint32_t band_rows, uint32_t band_stride_rows);
/* Number of rows the local buffer holds under the current banding (after padding to 8). */
uint32_t fs_local_rows(const fs_renderer *r);

/* Optional: render into caller-owned DEVICE memory (e.g. a torch tensor handed to RCCL) instead of the
 * internal buffer.  capacity_bytes = size of the caller's allocation: it must hold fs_local_rows() x rounded-width
 * elements of sizeof(IterType), otherwise hipErrorInvalidValue is returned and the internal buffer stays in use.
 * fs_init_memory with a new geometry drops the pointer; fs_set_row_bands re-validates it against the new banding
 * (and falls back to the internal buffer with an error when it is too small).  NULL restores the internal buffer. */
uint32_t fs_set_external_iter_buffer(fs_renderer *r, void *device_ptr, uint64_t capacity_bytes);
void *fs_device_iter_buffer(const fs_renderer *r);
uint32_t fs_rounded_width(const fs_renderer *r);
/* The sharded read-back of a row-tiled frame (this project's addition; the reference copies the whole iteration buffer through
 * its one device, GPURenderer::ExtractItersAndColors, GPU_Render.cu:1760-1805): the renderer's owned bands go straight to THEIR
 * rows of a whole-frame host buffer -- rows in frame order, row pitch = fs_rounded_width() x sizeof(IterType), (height padded to
 * 8) rows -- over this device's own PCIe link: one two-dimensional copy whose destination pitch is the band stride, so nothing has
 * to restore row order afterwards and no frame funnels through device 0.  device_iters = the buffer the frame was rendered into
 * (NULL = the renderer's current iteration buffer); stream = a hipStream_t of this device (NULL = the compute stream: behind the
 * kernel).  host_frame should be page-locked for every device that writes into it (hipHostMalloc with hipHostMallocPortable, or
 * fs_host_register -- e.g. a POSIX shared-memory frame that several rank processes fill); pageable memory works, synchronously.
 * Asynchronous.  Rows at and beyond the frame's height (the padding to 8) are only written without row bands, where the call is
 * the plain copy of the whole padded buffer. */
uint32_t fs_copy_bands_to_host(fs_renderer *r, const void *device_iters, void *host_frame, void *stream);
/* hipHostRegister (portable: usable by every device of the process) / hipHostUnregister of caller-owned host memory. */
uint32_t fs_host_register(void *host_ptr, uint64_t bytes);
uint32_t fs_host_unregister(void *host_ptr);

/* GPURenderer::InitializePerturb<IterType,T1,SubType,PExtras,T2> (GPU_Render.cu:431-501), split in two:
 * orbit upload (GPUPerturbSingleResults ctor, Perturb.cuh:20-80) ... */
uint32_t fs_upload_orbit(fs_renderer *r, uint64_t generation, int type_tag, uint32_t iter_bytes,
                         const void *entries, uint64_t orbit_size, uint64_t uncompressed_size,
                         uint64_t period_maybe_zero);
/* The same for PerturbExtras::SimpleCompression orbits: `entries` = GPUReferenceIter<T, SimpleCompression>[compressed_size]
 * (fs_orbit_hdr32_rc / _hdr64_rc / _f32_rc / _f64_rc / _p2x32_rc / _2x32_rc by type_tag), orbit_x_low / orbit_y_low =
 * GPUPerturbResults::OrbitXLow / OrbitYLow in the same numeric type (fs_real_hdr32 / fs_real_hdr64 / float / double /
 * fs_real_p2x32 / fs_real_2x32): the constant c of the runtime decompressor, Perturb.cuh:272-326.  The orbit is expanded
 * once on the device, in T arithmetic; all render calls then behave exactly as the reference's *RC* algorithms (for
 * HDRFloat<float|double>, float and double bit-identical to its CPU RuntimeDecompressor too).  All six numeric types. */
uint32_t fs_upload_orbit_compressed(fs_renderer *r, uint64_t generation, int type_tag, uint32_t iter_bytes,
                                    const void *entries, uint64_t compressed_size, uint64_t uncompressed_size,
                                    uint64_t period_maybe_zero, const void *orbit_x_low, const void *orbit_y_low);
/* How fs_upload_orbit_compressed keeps an orbit in HBM (set it before the upload; all six numeric types):
 *   0 (default)  expanded once on upload into the full orbit (fastest kernels; costs uncompressed_size entries of HBM);
 *   1            only the waypoints stay resident and every pixel decompresses the orbit as it walks it, with a sequential
 *                cursor -- GPUPerturbSingleResults::SeqWorkspace / GetIterSeq / BinarySearch (Perturb.cuh:146-326), the
 *                reason the format exists: orbits too long to hold expanded.  Same orbit values bit for bit, hence the same
 *                frames.  Served by fs_render_lav2 (all modes except perturbation-only with FS_PARITY_CPU, whose twin is the
 *                scalar kernel; every iteration cap -- 2^32 and above with a uint64_t iteration buffer); fs_render_bla /
 *                fs_build_la / fs_build_bla need the expanded orbit and return FS_ERR_UNSUPPORTED.  float / double / CudaDblflt /
 *                HDRFloat<CudaDblflt> orbits are walked the same way by their LAv2 kernels (GPU_Render.cu:518-523,532-537
 *                instantiates SimpleCompression for them too), with 32-bit positions.  For HDRFloat<float | double> orbit
 *                POSITIONS are IterType-wide like the reference's (Perturb.cuh:21-23,202-203,247-271; LAInfoI.h:5-19): an orbit of 2^32 and more uncompressed entries (only its waypoints are
 *                resident), a period, LA step lengths / next-stage indices and an AT step length beyond 32 bits are accepted
 *                -- fs_upload_la then keeps the uint64_t records as they are -- and the kernel walks them with 64-bit
 *                positions.  (Expanded orbits are limited to 2^32 - 1 entries: FS_ERR_UNSUPPORTED above that.)
 * fs_orbit_device_bytes: HBM bytes the resident orbit occupies in all its device forms (0 without an orbit). */
uint32_t fs_set_compressed_orbit_mode(fs_renderer *r, int mode);
uint64_t fs_orbit_device_bytes(const fs_renderer *r);
/* ... and LA table upload (GPU_LAReference ctor, GPU_LAReference.h:79-160).  at_info may be NULL when
 * use_at == 0.  iter_bytes selects the record family: 4 -> fs_la_*_u32 / fs_la_stage_u32 / fs_at_*_u32,
 * 8 -> fs_la_*_u64 / fs_la_stage_u64 / fs_at_*_u64 (narrowed on upload; kept as they are for HDRFloat<float | double> under
 * fs_set_compressed_orbit_mode(1) when a step length or index does not fit 32 bits). */
uint32_t fs_upload_la(fs_renderer *r, uint64_t generation, int type_tag, uint32_t iter_bytes, const void *las,
                      uint32_t n_las, const void *stages, uint32_t n_stages, int is_valid, int use_at,
                      const void *at_info);

/* The Feature Finder's perturbation evaluator (FeatureFinder::PTEvaluator::Eval, FeatureFinder.cpp:2313-2354, with
 * Evaluate_PT :1757-1958, PeriodicityPP :1471-1534 and the Direct fixed-period fallback Evaluate_PeriodResidualAndDzdc_Direct
 * :1661-1711) for n candidates at once, against the expanded orbit of fs_upload_orbit / fs_upload_orbit_compressed (the same
 * HBM copy the render kernels read).  mode FS_FEATURE_FIND: Eval<true> with cap max_iters; FS_FEATURE_FIXED: Eval<false> at
 * each candidate's period (PT, then Direct when PT escapes).  radius = R = HdrSqrt(SqrRadius) (fs_real_hdr32 / _hdr64);
 * in / out = fs_feature_in_* / fs_feature_out_* (fs_layout.h) by type_tag FS_T_HDR32 / FS_T_HDR64; iter_bytes = sizeof(IterType)
 * (4 or 8: the width periods are counted at).  Synchronous on the compute stream; n = 0 does nothing.  Frame state (iteration
 * buffer, recorded tile costs and orders, orbit / LA caches, kernel-time history) is left as it was.
 * FS_ERR_6: no orbit of this type resident.  FS_ERR_UNSUPPORTED: another type tag, iter_bytes or mode (FS_FEATURE_LA: the LA
 * evaluator is not built), or a waypoint-resident orbit (fs_set_compressed_orbit_mode(r, 1)): fs_feature_eval_resident serves
 * that one. */
enum { FS_FEATURE_FIND = 0, FS_FEATURE_FIXED = 1, FS_FEATURE_LA = 2 };
enum { FS_FEATURE_REJECTED = 0, FS_FEATURE_OK = 1, FS_FEATURE_OK_DIRECT = 2 };
uint32_t fs_feature_eval(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius, uint64_t max_iters,
                         const void *in, void *out, uint64_t n);
/* fs_feature_eval against the resident orbit in whichever form it is held (fs_orbit_form): the reference's Feature Finder for
 * PerturbExtras::SimpleCompression (FeatureFinder.cpp:2780-2795), whose Evaluate_PT walks the orbit through a RuntimeDecompressor
 * (:1757-1771).  The arguments, records, modes and result codes of fs_feature_eval.
 *   expanded orbit   the kernels of fs_feature_eval: the same records byte for byte;
 *   waypoints only   (fs_set_compressed_orbit_mode(r, 1)) every candidate walks the orbit with a decompression cursor of its own
 *                    (c = the OrbitXLow / OrbitYLow of the upload, count = the uncompressed size).  Both forms see the same
 *                    orbit bit for bit, hence the same records.  Orbit positions are IterType-wide as the reference's are
 *                    (Perturb.cuh:21-23, 202-203): iter_bytes = 8 serves an orbit of 2^32 entries and more.
 * Synchronous on the compute stream; slices through fs_set_feature_slice; n = 0 returns 0; frame state is left as it was.
 * FS_ERR_UNSUPPORTED: another type tag, iter_bytes or mode, or a waypoint-resident orbit of 2^32 entries and more with
 * iter_bytes = 4.  FS_ERR_6: no orbit of this type resident.  hipErrorInvalidValue: a NULL argument, or a fixed period that a
 * 4-byte IterType cannot hold.
 * fs_orbit_form: 0 = no orbit resident, 1 = expanded, 2 = waypoints only. */
uint32_t fs_feature_eval_resident(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius,
                                  uint64_t max_iters, const void *in, void *out, uint64_t n);
int fs_orbit_form(const fs_renderer *r);
/* FeatureFinder::DirectEvaluator::Eval (FeatureFinder.cpp:2188-2211) for n candidates: FS_FEATURE_FIND = Evaluate_FindPeriod_Direct
 * (:1576-1660: the trigger |z|^2 < R^2 |dzdc|^2 with the fixed R of the call, cap max_iters), FS_FEATURE_FIXED =
 * Evaluate_PeriodResidualAndDzdc_Direct at each candidate's period; no fallback.  The records of fs_feature_eval: reads `c` and,
 * when fixed, `period`; ignores `dc`.  status FS_FEATURE_OK_DIRECT, or FS_FEATURE_REJECTED with an all-zero record.
 * Needs no resident orbit, no LA table and no fs_init_memory (a renderer fresh from fs_create will do); with a frame and an orbit
 * present it leaves them, and all frame state named above, as they were.  Synchronous on the compute stream; n = 0 returns 0 and
 * launches nothing.  FS_ERR_UNSUPPORTED: type tags other than FS_T_HDR32 / FS_T_HDR64, iter_bytes not 4 or 8, a mode other than
 * FS_FEATURE_FIND / FS_FEATURE_FIXED.  hipErrorInvalidValue: a fixed period that a 4-byte IterType cannot hold. */
uint32_t fs_feature_eval_direct(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius,
                                uint64_t max_iters, const void *in, void *out, uint64_t n);
/* The Feature Finder for the plain numeric types, T = float (FS_T_F32) / double (FS_T_F64): what the reference runs when the
 * render algorithm's MainType is plain (FeatureFinderOrchestrator.cpp:457-469, FeatureFinder.cpp:2740-2795), Gpu1x32PerturbedLAv2*
 * -- its automatic choice below a zoom factor of 1e34 -- among them.  C = FloatComplex<T>, every operation one IEEE operation.
 * The calls above keep refusing these two tags; these two refuse every other.
 *   fs_feature_eval_plain         PTEvaluator::Eval<true | false> against the resident plain orbit of that type (fs_upload_orbit /
 *                                 fs_upload_orbit_compressed with FS_T_F32 / FS_T_F64) in whichever form it is held
 *                                 (fs_orbit_form): expanded, one lane per candidate; waypoints only
 *                                 (fs_set_compressed_orbit_mode(r, 1)), a decompression cursor per lane with positions as wide as
 *                                 iter_bytes.  Both forms give the same records byte for byte.
 *   fs_feature_eval_plain_direct  DirectEvaluator::Eval; needs no orbit and no fs_init_memory.
 * radius = R as one float / double (HdrSqrt(SqrRadius), computed by the host); in / out = fs_feature_in_f32 / _f64,
 * fs_feature_out_f32 / _f64 (fs_layout.h); modes, statuses and iter_bytes as fs_feature_eval.  Synchronous on the compute stream;
 * slices through fs_set_feature_slice; n = 0 returns 0 without a launch; frame state, caches and kernel-time history are left
 * as they were.
 * FS_ERR_UNSUPPORTED: another type tag, iter_bytes not 4 or 8, mode FS_FEATURE_LA or unknown, a waypoint-resident orbit of 2^32
 * entries and more with iter_bytes = 4.  FS_ERR_6 (fs_feature_eval_plain only): no orbit of this type resident.
 * hipErrorInvalidValue: a NULL argument, or a fixed period that a 4-byte IterType cannot hold. */
uint32_t fs_feature_eval_plain(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius,
                               uint64_t max_iters, const void *in, void *out, uint64_t n);
uint32_t fs_feature_eval_plain_direct(fs_renderer *r, int type_tag, uint32_t iter_bytes, int mode, const void *radius,
                                      uint64_t max_iters, const void *in, void *out, uint64_t n);

/* The AutoZoomer's choice of the next zoom target (AutoZoomer::Run, AutoZoomer.cpp:74-393) on the device, from the iteration
 * buffer the render kernels wrote: the frame is never read back.  W x H below = the frame of fs_init_memory (antialiasing
 * included), row 0 = the buffer's row 0.  device_iters: another device buffer of the same geometry and IterType, NULL = the
 * renderer's current one.  out = fs_autozoom_result (fs_layout.h), which says per heuristic what every field holds.
 *   FS_AUTOZOOM_MAX           the first pixel in raster order that holds the frame's largest count (zoom divisor 32)
 *   FS_AUTOZOOM_FILAMENT_TIP  the best-scoring filament tip inside the 18-pixel margin (divisor 8).  Classification and counts
 *                             are integer work on the device; the score involves log(), which the device does not compute as the
 *                             host's libm does, so the device score only SELECTS candidates: every accepted candidate within
 *                             2^-40 of the device maximum is re-scored on the host with libm, in raster order, strict `>`.
 *   FS_AUTOZOOM_DEFAULT       the weighted mean position over the inner rectangle (divisor 3).  Its three sums are non-integer
 *                             doubles: summed in a fixed tree (bitwise equal from run to run), not in the reference's raster
 *                             order -- target_x / target_y agree with a sequential sum to 4 n 2^-53 relative, n = pixels of the
 *                             rectangle.
 * status follows the reference's order of tests: FS_AUTOZOOM_FLAT = Max / Default "flat screen", and FilamentTip's stop on
 * num_at_max > W H / 2 (none of them moves); FS_AUTOZOOM_NO_TARGET = FilamentTip without an accepted candidate (or an all-zero
 * frame); FS_AUTOZOOM_MOVE_THEN_STOP = Max / Default with num_at_max > 500: move, then stop.
 * Sums of counts are integers on the device, converted to double once: the reference's running double sum rounds on the way once
 * it passes 2^53, this one does not (no test goes there).
 * Synchronous on the compute stream, behind the render.  Frame state (iteration buffer, recorded tile costs and orders, orbit / LA
 * caches, kernel-time history) is left as it was.  FS_ERR_6: no fs_init_memory yet.  FS_ERR_UNSUPPORTED: row bands set
 * (fs_set_row_bands), an unknown heuristic, a frame smaller than the heuristic's margins (FilamentTip: W or H <= 36). */
enum { FS_AUTOZOOM_DEFAULT = 0, FS_AUTOZOOM_MAX = 1, FS_AUTOZOOM_FILAMENT_TIP = 2 };
enum { FS_AUTOZOOM_MOVE = 0, FS_AUTOZOOM_MOVE_THEN_STOP = 1, FS_AUTOZOOM_FLAT = 2, FS_AUTOZOOM_NO_TARGET = 3 };
uint32_t fs_autozoom_pick(fs_renderer *r, int heuristic, uint64_t n_iterations, const void *device_iters,
                          fs_autozoom_result *out);

/* BLA table upload (GPU_BLAS ctor, BLA.cuh:123-160); the reference does this inside RenderPerturbBLA. */
uint32_t fs_upload_bla(fs_renderer *r, int type_tag, const void *const *levels, const uint64_t *level_sizes,
                       int32_t n_levels, int32_t lm2);

/* BLAS<IterType,T>::Init(count, blaSize) (FractalSharkLib/BLAS.cpp:212-255) executed on the device instead of the host:
 * builds the BLA table of the orbit last uploaded with fs_upload_orbit (type_tag FS_T_HDR32 / FS_T_HDR64) directly in
 * HBM and installs it as the renderer's table, bit-identical to the host builder.  bla_size = the orbit's max radius
 * (fs_real_hdr32 / fs_real_hdr64, PerturbationResults::GetMaxRadius, Fractal.cpp:2739-2740).  Asynchronous on the compute
 * stream.  The reference rebuilds this table on the CPU and copies it over PCIe on every BLA render. */
uint32_t fs_build_bla(fs_renderer *r, int type_tag, const void *bla_size);

/* LAReference::GenerateApproximationData (FractalSharkLib/LAReference.cpp:971-1013: CreateLAFromOrbit :28-210,
 * CreateNewLAStage :774-966, CreateATFromLA :1050-1074) executed on the DEVICE instead of the host: builds the LAv2 table
 * (all stages + ATInfo) of the orbit last uploaded with fs_upload_orbit / fs_upload_orbit_compressed (type_tag FS_T_HDR32 /
 * FS_T_HDR64) directly in HBM and installs it as the renderer's table, as fs_upload_la would.  max_radius =
 * PerturbationResults::GetMaxRadius (fs_real_hdr32 / fs_real_hdr64); use_small_exponents = the UseSmallExponents flag of
 * CreateATFromLA (RefOrbitCalc.cpp:2346).  The table is bit-identical to the reference's SINGLE-THREADED builder (what
 * LAReference produces when hardware_concurrency() < 2 or the orbit has fewer than 2 * 50000 entries, :236-251; the
 * multi-threaded stage-0 variant yields a thread-count-dependent table: fs_build_la_mt below).  An orbit of at most 64 steps (LowBound,
 * LAReference.h:56) in which no period is found gets the reference's two records and a table that is not valid (:135-140,
 * :1002-1005; fs_la_counts reports is_valid 0 and the kernels ignore the table); one in which periods are found gets its
 * normal small table.  FS_ERR_UNSUPPORTED (use fs_upload_la): an orbit of fewer than three entries, a first step whose ZCoeff
 * is zero.  Synchronous.  (fs_la_counts / fs_read_la of fsmi355_internal.h read the installed table back: tests, tools.) */
uint32_t fs_build_la(fs_renderer *r, int type_tag, const void *max_radius, int use_small_exponents);
/* ... and with stage 0 as LAReference::CreateLAFromOrbitMT (LAReference.cpp:215-770) builds it on a host with `host_threads`
 * hardware threads (std::thread::hardware_concurrency(), :236-240): ThreadCount = min(maxRefIteration / 50000, host_threads)
 * pieces -- the Starter from the prologue, Worker k from the first period boundary it finds after orbit index
 * maxRefIteration * k / ThreadCount (:486-560), each until it meets the next published start (:640-668), stitched (:711-760) --
 * so that the table is, bit for bit, the one FractalShark's own CPU builder makes on THAT host (it differs from the
 * single-threaded table near every piece boundary).  ThreadCount < 2 (host_threads < 2 or an orbit below 100 000 entries) is
 * fs_build_la.  The device computes next() for every state of the scan and the 2 (ThreadCount - 1) uncapped first detections;
 * the host walks the chains (indices only: 8 bytes per orbit entry come back once) and stitches; the device folds the records. */
uint32_t fs_build_la_mt(fs_renderer *r, int type_tag, const void *max_radius, int use_small_exponents, int host_threads);

/* GPURenderer::RenderPerturbLAv2<IterType,T,SubType,Mode,PExtras> (GPU_Render.cu:995-1188) for all six numeric types of
 * its instantiation list (:1204-1300): FS_T_HDR32 / FS_T_HDR64 / FS_T_HDR2X32 (GpuHDRx32 / x64 / x2x32 PerturbedLAv2*)
 * and the non-HDR FS_T_F32 / FS_T_F64 / FS_T_2X32 (Gpu1x32 / Gpu1x64 / Gpu2x32 PerturbedLAv2*; orbit, table and ATInfo
 * in the "plain" record families of fs_layout.h, uploaded with the same type_tag).
 * coords = {dx, dy, centerX, centerY} in the type selected by type_tag (fs_real_hdr32[4], fs_real_hdr64[4],
 * fs_real_2x32[4], float[4], double[4], fs_real_p2x32[4]).  `parity` only applies to FS_T_HDR32 / FS_T_HDR64 (the types
 * with a CPU twin).  Asynchronous on the compute stream. */
uint32_t fs_render_lav2(fs_renderer *r, int type_tag, int mode, int parity, const void *coords,
                        uint64_t n_iterations);

/* GPURenderer::RenderPerturbBLA<IterType,T> (GPU_Render.cu:1440-1607); uses the orbit of fs_upload_orbit and
 * the table of fs_upload_bla (n_levels == 0 there = plain perturbation). */
uint32_t fs_render_bla(fs_renderer *r, int type_tag, const void *coords, uint64_t n_iterations);

/* GPURenderer::Render<IterType,T> (GPU_Render.cu:617-846), direct escape-time kernels.
 * coords = {dx, dy, minX, maxY} (doubles for FS_T_F64), CPU twin Fractal::CalcCpuHDR (Fractal.cpp:2096-2206). */
uint32_t fs_render_direct(fs_renderer *r, int type_tag, const void *coords, uint64_t n_iterations);

/* GPURenderer::RenderPerturbBLAScaled<IterType,T> (GPU_Render.cu:1302-1376) -> mandel_1x_float_perturb_scaled
 * (ScaledKernels.cuh:3-239), T = HDRFloat<float> (FS_T_HDR32, RenderAlgorithm GpuHDRx32PerturbedScaled).
 * fs_upload_orbit_scaled takes the two PerturbExtras::Bad orbits the reference passes into the render call:
 * entries_t = GPUReferenceIter<HDRFloat<float>,Bad>[n] (fs_orbit_hdr32_bad), entries_f32 = GPUReferenceIter<float,Bad>[n]
 * (fs_orbit_f32_bad).  coords = fs_real_hdr32{dx, dy, centerX, centerY}.  No CPU RenderAlgorithm exists for this path:
 * the kernel restates the reference's CUDA kernel with un-contracted IEEE binary32 arithmetic. */
uint32_t fs_upload_orbit_scaled(fs_renderer *r, int type_tag, uint32_t iter_bytes, const void *entries_t,
                                const void *entries_f32, uint64_t orbit_size, uint64_t period_maybe_zero);
uint32_t fs_render_scaled(fs_renderer *r, int type_tag, const void *coords, uint64_t n_iterations);

/* GPURenderer::Render<IterType,T> for the direct kernels that have no CPU RenderAlgorithm twin (LowPrecisionKernels.cuh):
 * FS_T_F32 -> mandel_1x_float (Gpu1x32), coords = float{cx, cy, dx, dy};  FS_T_2X32 -> mandel_2x_float (Gpu2x32),
 * coords = float{cx.head, cx.tail, cy.head, cy.tail, dx.head, dx.tail, dy.head, dy.tail} (MattDblflt);  FS_T_2X64 ->
 * mandel_2x_double (Gpu2x64), the same eight values as doubles (MattDbldbl);  FS_T_4X32 -> mandel_4x_float (Gpu4x32),
 * coords = float{cx.x..w, cy.x..w, dx.x..w, dy.x..w} (MattQFltflt, most significant first);  FS_T_4X64 -> mandel_4x_double
 * (Gpu4x64), the same sixteen values as doubles (MattQDbldbl).  cx / cy = the view's MIN corner
 * (Fractal::FillGpuCoords, Fractal.cpp:1833-1844); rows are written flipped like the reference.  iteration_precision in
 * {1, 4, 8, 16} (ignored by Gpu2x64 / Gpu4x32 / Gpu4x64); other values launch nothing and return 0, like the reference's switch.  The kernels
 * restate the CUDA kernels (no CPU twin exists; un-contracted IEEE arithmetic, __fmaf_rd = fma rounded toward -inf). */
uint32_t fs_render_direct_lp(fs_renderer *r, int type_tag, const void *coords, uint64_t n_iterations,
                             int iteration_precision);

/* The exact renderer (this project's addition; the render path of the reference's CpuHigh, CalcCpuHDR<IterType, HighPrecision,
 * double>, Fractal.cpp:1200-1201, 2096-2206, at any depth and without a reference orbit).  Every sample is iterated in
 * fixed point with frac_bits fractional bits on integers of `limbs` 32-bit limbs,
 *     x' = floor((x^2 - y^2) / 2^F) + cx,   y' = floor(2 x y / 2^F) + cy,   escape when x^2 + y^2 > R 2^2F (>= when inclusive),
 * with no rounding anywhere: the frame equals GMP integer iteration of the same recurrence on every pixel.
 * cx, cy: the axes, c * 2^F as two's-complement numbers of `limbs` limbs, limb-major over the W x H of fs_init_memory
 * (cx[l * W + x], cy[l * H + y]; fsh_view_exact_axes of fs_inputs.h makes them).  bailout = R, an integer.
 * The frame is an ordinary one in the renderer's iteration buffer: with E the first n >= 1 with |z_n|^2 > R (z_1 = c), a pixel
 * holds min(E - 1, n_iterations), and n_iterations when there is no escape within n_iterations + 1 -- the convention of every
 * other path.  fs_render_current, the reductions and fs_autozoom_pick work on it unchanged.  Synchronous on the compute stream; the
 * orbit and LA caches, recorded tile costs and orders and the kernel-time history are left as they were.
 * FS_ERR_6: no fs_init_memory yet.  FS_ERR_UNSUPPORTED: row bands set (fs_set_row_bands); iter_bytes not 4 or 8; limbs outside
 * 2 .. 24 or 32 * limbs < frac_bits + 10 (so frac_bits <= 758); bailout outside 1 .. 256; an axis value outside [-32, 32).
 * hipErrorInvalidValue: iter_bytes is not the frame's, a NULL axis, an n_iterations the frame's IterType cannot hold. */
uint32_t fs_render_exact(fs_renderer *r, uint32_t iter_bytes, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx,
                         const uint32_t *cy, uint32_t bailout, int inclusive, uint64_t n_iterations);
/* Which pixels of the exact frame in the iteration buffer (the centre frame, rendered with the same frac_bits, bailout and
 * n_iterations, strict bailout) keep their count when c moves by s: cx[3], cy[3] = the axes {c, c + s, c - s} (fsh_view_exact_axes
 * with a shift level).  The four frames at c + s, c - s, c + is, c - is are rendered into scratch memory and compared with the
 * centre frame on the device; host_mask[y * W + x] = 1 where all four equal it, else 0.  The iteration buffer is not written.
 * Synchronous; errors as fs_render_exact. */
uint32_t fs_exact_stable_mask(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *const cx[3],
                              const uint32_t *const cy[3], uint32_t bailout, uint64_t n_iterations, uint8_t *host_mask);
/* The wide exact renderer: the same recurrence, counting and limb bound with one 64-lane wave per sample, each lane holding
 * ceil(limbs / 64) limbs of every number, for limbs = 2 .. 704 (frac_bits <= 22518; DESIGN.md 6.3 "Wide").  A count equals
 * fs_render_exact's wherever both accept the call.
 * fs_exact_sample_counts: n_samples samples of their own, cx[l * n_samples + i] and cy[l * n_samples + i] (limb-major per SAMPLE);
 * counts_out[i] = min(E - 1, n_iterations), host memory.  Synchronous.  Needs no frame and no fs_init_memory (the streams are made
 * if they are missing); the iteration buffer, orbit and tables are left alone.  A lattice with its stability ladder is five calls
 * per level.
 * fs_render_exact_wide: the arguments of fs_render_exact and its frame, for limbs = 2 .. 704.
 * Errors as fs_render_exact with 704 in place of 24 (fs_exact_sample_counts has no frame: no FS_ERR_6, no row bands, no iter_bytes);
 * hipErrorInvalidValue also for more than 2^31 - 1 samples or pixels (one workgroup each). */
uint32_t fs_exact_sample_counts(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                                uint32_t n_samples, uint32_t bailout, int inclusive, uint64_t n_iterations, uint64_t *counts_out);
uint32_t fs_render_exact_wide(fs_renderer *r, uint32_t iter_bytes, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx,
                              const uint32_t *cy, uint32_t bailout, int inclusive, uint64_t n_iterations);
/* Point runs: the exact recurrence on a list of points with a length each, the state at the end of every run and the period rule
 * (DESIGN.md 6.3 "Point runs"; what exact.refine_points refines the Feature Finder's found points with).  One lane per run,
 * limbs = 2 .. 24.  Run e: c = (cx[l * n_runs + e], cy[l * n_runs + e]) (limb-major per RUN, as fs_exact_sample_counts) and
 * p = lengths[e] >= 1.  With z_1 = c, N_n = x_n^2 + y_n^2 untruncated and E the first n at which z_n escapes:
 *   values_out[e] = v = min(E - 1, p);
 *   atoms_out[e]  = the n in 1 .. v with the smallest N_n, ties to the earliest n; 0 when v = 0;
 *   end_x_out[l * n_runs + e], end_y_out[l * n_runs + e] = limb l of x_p, y_p when v == p, else 0 on every limb.
 * All four are host memory; every value equals the recurrence on integers, whatever the slices and the compaction (runs of
 * different lengths leave the list at different slices).  Synchronous.  Needs no frame and no fs_init_memory; the iteration buffer,
 * the orbit and LA caches, the kept set and the period planes of the last fs_render_exact are left alone.  The cycle-check, keep and
 * periods switches are not read.  fs_set_exact_slice applies (default: as for the lists of fs_exact_audit); fs_read_exact_stats
 * reports the call.  n_runs == 0: 0.
 * FS_ERR_UNSUPPORTED: limbs outside 2 .. 24 or 32 * limbs < frac_bits + 10; bailout outside 1 .. 256; a c outside [-32, 32).
 * hipErrorInvalidValue: a NULL pointer; a length of 0 or 2^64 - 1; more than 2^31 - 1 runs. */
uint32_t fs_exact_eval_points(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                              const uint64_t *lengths, uint32_t n_runs, uint32_t bailout, int inclusive, uint64_t *values_out,
                              uint64_t *atoms_out, uint32_t *end_x_out, uint32_t *end_y_out);
/* fs_exact_eval_points through the wide kernels: one wave per run at every limb count, limbs = 2 .. 704 (frac_bits <= 22518; DESIGN.md
 * 6.3 "Point runs on the wide path").  The arguments, the layouts and every value are fs_exact_eval_points': wherever both accept a
 * call their outputs are equal byte for byte.  Synchronous.  Needs no frame and no fs_init_memory; the iteration buffer, the orbit
 * and LA caches, the kept set and the period planes of the last fs_render_exact are left alone, and no switch is read.
 * fs_set_exact_slice applies (default: the wide path's, about 50 ms of a lone wave); fs_read_exact_stats reports the call as the
 * wide path does, 64 lane slots per step of a wave.  n_runs == 0: 0.
 * FS_ERR_UNSUPPORTED: limbs outside 2 .. 704 or 32 * limbs < frac_bits + 10; bailout outside 1 .. 256; a c outside [-32, 32).
 * hipErrorInvalidValue: a NULL pointer; a length of 0 or 2^64 - 1; more than 2^31 - 1 runs. */
uint32_t fs_exact_eval_points_wide(fs_renderer *r, uint32_t frac_bits, uint32_t limbs, const uint32_t *cx, const uint32_t *cy,
                                   const uint64_t *lengths, uint32_t n_runs, uint32_t bailout, int inclusive, uint64_t *values_out,
                                   uint64_t *atoms_out, uint32_t *end_x_out, uint32_t *end_y_out);
/* The exact audit: the project's definition of a correct frame -- equal to the exact count on every sample that is stable at a
 * stated level -- as one call on the frame in the iteration buffer (device_iters: another device buffer of the same
 * geometry and IterType, NULL = the current one).  n_samples sample pixels (xs[i], ys[i]) of the W x H of fs_init_memory and a
 * ladder of n_levels <= FS_AUDIT_MAX_LEVELS shifts give n_samples * (1 + 4 n_levels) runs of the exact recurrence above:
 * cx_runs, cy_runs = [1 + 4 n_levels][limbs][n_samples] (host), run 0 = c and run 1 + 4 j + d = c + s_j, c - s_j, c + i s_j,
 * c - i s_j for d = 0 .. 3.  All runs of a call are ONE list that fills the chip and compacts together: one lane per run for
 * limbs = 2 .. 24, one wave per run beyond, up to 704.  A second kernel reads the frame at the samples, next to it, and reduces
 * everything to *out (fs_layout.h): exact = the count of run 0, bit j of stable_bits = the four counts of level j equal it, differ =
 * frame != exact.  Integers only; the same record from run to run.  Only the record crosses the bus, and whichever of
 * exact_out[n_samples], frame_out[n_samples], stable_out[n_samples] (the stable_bits) are not NULL.
 * The rule is min(E - 1, n_iterations): the perturbation families (bailout 256) and the direct kernels that have a CPU twin
 * (bailout 4).  The low-precision direct kernels of fs_render_direct_lp count differently (a row shift, multiples of
 * iteration_precision): their frames are out of scope.
 * Synchronous on the compute stream; the frame, the orbit and LA caches, recorded tile costs and orders and the kernel-time history
 * are left as they were.  fs_read_exact_stats reports the call's lane slots, steps and launches.  n_samples == 0: 0 and a zeroed
 * record.
 * FS_ERR_6: no fs_init_memory yet.  FS_ERR_UNSUPPORTED: row bands set; limbs outside 2 .. 704 or 32 * limbs < frac_bits + 10;
 * bailout outside 1 .. 256; n_levels > 8; an axis value outside [-32, 32).  hipErrorInvalidValue: NULL xs, ys, cx_runs, cy_runs
 * or out; a sample outside the frame; more than 2^31 - 1 runs; an n_iterations the frame's IterType cannot hold. */
uint32_t fs_exact_audit(fs_renderer *r, const void *device_iters, uint32_t frac_bits, uint32_t limbs, const uint32_t *xs,
                        const uint32_t *ys, uint32_t n_samples, uint32_t n_levels, const uint32_t *cx_runs, const uint32_t *cy_runs,
                        uint32_t bailout, int inclusive, uint64_t n_iterations, fs_audit_result *out, uint64_t *exact_out,
                        uint64_t *frame_out, uint32_t *stable_out);

/* The exact renderer's cycle check: a proof of non-escape by an exact repeat of the state (DESIGN.md 6.3 "Cycle check").  The
 * recurrence is integer and nothing is rounded, so a sample whose z_n equals, limb for limb, a z_m it held before (m < n) walks a
 * cycle of states that have all passed the escape test: it escapes at no cap, and it leaves the loop with n_iterations as its value
 * at once instead of after n_iterations + 1 steps.  No pixel changes.  Every sample keeps one checkpoint, z_1 = c at first and
 * retaken at every n that is a power of two.
 * fs_set_exact_cycle_check: enable = 1 switches the check on for fs_render_exact, the four shifted frames of fs_exact_stable_mask
 * and fs_exact_audit up to 24 limbs (the running samples then carry 2 * limbs more limb planes); 0, the default, off: every call
 * does exactly what it does without this function.  fs_render_exact_wide, fs_exact_sample_counts and fs_exact_audit beyond 24
 * limbs ignore the switch.  What the check cannot prove within the cap -- long periods, samples near a component's boundary,
 * parabolic ones -- runs to the cap as before.
 * fs_read_exact_proved: out[n] (host) = 1 for the samples the last call finished by proof: of the last fs_render_exact, row-major
 * over the W x H of fs_init_memory (n = W * H); of the last fs_exact_audit, its runs in run order (n = n_samples * (1 + 4
 * n_levels), run k of sample i at k * n_samples + i).  fs_exact_stable_mask with the check on leaves the mask of the frame before
 * it.  FS_ERR_6: the last exact call ran with the check off (or there was none); hipErrorInvalidValue: n is not the mask's size. */
uint32_t fs_set_exact_cycle_check(fs_renderer *r, int enable);
uint32_t fs_read_exact_proved(const fs_renderer *r, uint8_t *out, uint64_t n);

/* Continuation: raise the cap of the exact frame in the iteration buffer without starting over (DESIGN.md 6.3 "Continuation").
 * z_{n+1} is a function of z_n alone, so a sample's state at step N is the same whatever cap the call was given, and a larger cap
 * is one more slice boundary.
 * fs_set_exact_keep: enable = 1 makes fs_render_exact and fs_render_exact_wide leave a kept set on the device when they return:
 * the state of every sample that reached the cap without escaping and without a proof, the proved plane (cycle check on), the two
 * axes and the call's parameters.  The set is sized to the samples kept, not to W x H, and replaces any earlier one; it is no idle
 * memory (fs_release_idle_device_memory leaves it).  A failed allocation while keeping is the call's error.  0, the default: no set
 * is left and every call does exactly what it does without this function.  The switch is read by the two renderers only:
 * switching it off neither frees a set that exists nor keeps fs_render_exact_continue from continuing it and keeping again.
 * fs_render_exact_continue: resumes the kept samples up to n_iterations = N2 >= the kept cap N1, with the path, the parameters and
 * the cycle-check setting recorded with the set (not the current switches).  Afterwards the iteration buffer is, byte for byte,
 * what the original call with n_iterations = N2 writes from scratch -- the proved pixels are rewritten to N2 -- and the kept set
 * is that of cap N2: calls chain.  fs_read_exact_proved returns the mask a fresh call at N2 would give; fs_read_exact_stats and
 * fs_read_exact_cycle_stats report this call's work only (a resumed sample of the wide path repeats one escape test).  Synchronous
 * on the compute stream; the orbit and LA caches, recorded tile costs and orders and the kernel-time history are left as they
 * were.  N2 == N1: 0, nothing changes.  Nothing kept and nothing proved (every pixel escaped): 0 without a launch, N2 recorded.
 * FS_ERR_6: no valid kept set.  hipErrorInvalidValue: N2 < N1, N2 == ~0, N2 > 2^32 - 1 on a 4-byte frame.  A continuation that
 * fails on its first allocation, before it has touched the frame or the set, leaves both as they were; one that fails later drops
 * the set.
 * fs_exact_kept_info: *out (fs_layout.h) describes the kept set; zeroed, and 0 returned, when nothing is kept.
 * fs_exact_drop_kept: frees the kept set.
 * The set describes the frame in the iteration buffer, so whatever writes, clears or replaces that buffer drops it at call time:
 * fs_init_memory, fs_clear, fs_set_row_bands, fs_set_external_iter_buffer, every fs_render_* into the buffer (the two exact ones
 * replace it when keep is on and drop it when off) and fs_destroy.  fs_render_current, fs_colorize_frame, fs_autozoom_pick,
 * fs_exact_audit, fs_exact_stable_mask, fs_exact_sample_counts, fs_feature_eval* and the stream calls leave it alone. */
uint32_t fs_set_exact_keep(fs_renderer *r, int enable);
uint32_t fs_render_exact_continue(fs_renderer *r, uint64_t n_iterations);
uint32_t fs_exact_kept_info(const fs_renderer *r, fs_exact_kept *out);
uint32_t fs_exact_drop_kept(fs_renderer *r);

/* Period planes: the exact family's own period map (DESIGN.md 6.3 "Period planes").  n is the index of the z a sample holds,
 * z_1 = c; a pixel's value is v = min(E - 1, n_iterations).  Both planes are integers defined on the exact recurrence; they are NOT
 * the Feature Finder's trigger |z|^2 < R^2 |dzdc|^2 and claim no equality with its evaluators.
 * Atom period A: the n in 1 .. v with the smallest untruncated norm x_n^2 + y_n^2 (the 2 * limbs-limb sum the escape test is made
 * on), ties to the earliest n; 0 when v = 0.  Only states that passed the escape test with n <= n_iterations are tracked, so
 * A <= v.  Inside the atom domain of a period-p nucleus it is p.  A does not depend on the cycle check, the slices or compaction.
 * Cycle length: for a sample the cycle check proves at index n, n - t, t the index its checkpoint was taken at (the largest power
 * of two below n): a multiple of the cycle's period.  0 for a sample that is not proved.
 * fs_set_exact_periods: enable = 1 makes fs_render_exact (up to 24 limbs) leave the atom plane and, with the cycle check on, the
 * cycle-length plane besides the frame, which is byte for byte the frame without the switch; the call's device block grows by
 * 2 * limbs + 4 (+ 2 with the cycle check) words per pixel.  0, the default: the same kernels run as without this function and
 * nothing more is allocated.  With the switch AND fs_set_exact_keep on, fs_render_exact returns FS_ERR_UNSUPPORTED before it touches
 * the frame or the kept set.  Every other exact entry point -- fs_exact_stable_mask, fs_exact_sample_counts, fs_exact_audit,
 * fs_render_exact_wide, fs_render_exact_continue -- ignores the switch and leaves the planes of the last fs_render_exact alone.
 * fs_read_exact_atom_periods / fs_read_exact_cycle_lengths: out[n] (host), n = W * H of fs_init_memory, row-major.  FS_ERR_6: the
 * last fs_render_exact ran with the switch off (the cycle lengths: with the switch or the cycle check off), failed, or there was
 * none; hipErrorInvalidValue: NULL, or n is not the plane's size. */
uint32_t fs_set_exact_periods(fs_renderer *r, int enable);
uint32_t fs_read_exact_atom_periods(const fs_renderer *r, uint64_t *out, uint64_t n);
uint32_t fs_read_exact_cycle_lengths(const fs_renderer *r, uint64_t *out, uint64_t n);

/* GPURenderer::ClearMemory<IterType> (GPU_Render.cu:212-225). */
uint32_t fs_clear(fs_renderer *r);

/* GPURenderer::RenderCurrent<IterType> (GPU_Render.cu:556-581): antialias + palette, min/max/sum, D2H.
 * Any of the three host pointers may be NULL.  progressive != 0 runs on the display stream. */
uint32_t fs_render_current(fs_renderer *r, uint64_t n_iterations, void *iter_buffer, fs_color16 *color_buffer,
                           fs_reduction *reduction, int progressive);

/* RenderCurrent's colour half (RunAntialiasing, GPU_Render.cu:1695-1757) over a whole frame that lies elsewhere on the
 * renderer's device -- the frame an fs_group has gathered and put back in row order: antialias + palette with this renderer's
 * palette and geometry into device_colors (NULL = the renderer's own colour buffer), then, if color_buffer is not NULL, the
 * copy of N_color_cu Color16 to the host, all on `stream` (a hipStream_t of that device).  fs_color_buffer_elements =
 * N_color_cu, the element count of a colour buffer (padded to 16 x 8 blocks like the reference's). */
uint32_t fs_colorize_frame(fs_renderer *r, const void *device_iters, uint64_t n_iterations, fs_color16 *device_colors,
                           fs_color16 *color_buffer, void *stream);
uint64_t fs_color_buffer_elements(const fs_renderer *r);

/* SyncComputeStream / SyncDisplayStream / QueryComputeStream / EnqueueComputeDoneCallback
 * (GPU_Render.cu:596-615).  The callback runs on a runtime thread after all prior compute-stream work. */
uint32_t fs_sync_compute(fs_renderer *r);
uint32_t fs_sync_display(fs_renderer *r);
/* The compute stream itself (a hipStream_t; GPURenderer::m_ComputeStream, GPU_Render.h), NULL before fs_init_memory.  For a
 * host that chains its own device work behind a render without a host round trip (the multi-GPU gather of bench.py waits
 * on it from its own stream).  Owned by the renderer. */
void *fs_compute_stream(const fs_renderer *r);
/* The display stream (GPURenderer::m_DisplayStream: high priority, where a progressive RenderCurrent runs). */
void *fs_display_stream(const fs_renderer *r);
uint32_t fs_query_compute(fs_renderer *r);
typedef void (*fs_done_cb)(void *user);
uint32_t fs_enqueue_done_callback(fs_renderer *r, fs_done_cb cb, void *user);

/* Memory behaviour (GPU_Render.cu:127,142-153,362-395; Perturb.cuh:51-61; GPU_LAReference.h:93-113): device memory is
 * allocated with hipMalloc / hipFree behind a synchronisation of the compute stream (FSMI355_ASYNC_ALLOC=1 in the environment
 * selects hipMallocAsync / hipFreeAsync in compute-stream order instead -- off by default); the work memory of fs_build_la, the installed
 * LA table and the BLA table (one allocation for all levels) are kept and reused when the next one fits.  When the device
 * cannot hold an INPUT table (reference orbit, LA table, BLA table) it is placed in page-locked host memory instead and the
 * kernels read it over the bus, as the reference does -- the frame still renders, slowly.  fs_host_fallback_bytes = bytes
 * ever placed there by this renderer (0 in normal operation).  FSMI355_FAIL_INPUT_ALLOC=1 in the environment when
 * fs_create runs makes every input allocation of that renderer take the fallback (fault injection for tests). */
uint64_t fs_host_fallback_bytes(const fs_renderer *r);
/* Device memory a renderer keeps idle for its next allocation (blocks it has freed: at most 16 blocks / 2 GiB, reused when
 * the next request fits).  A renderer whose allocation fails frees its own idle blocks, then those of EVERY renderer of the
 * process on the same device (FractalShark holds four GPURenderers on one device), and only then takes the page-locked
 * fallback or reports the error.  fs_idle_device_bytes: what `r` holds idle now; fs_release_idle_device_memory: frees the idle
 * blocks of all renderers on `device` (what the out-of-memory path does), returns the bytes freed.  Thread-safe. */
uint64_t fs_idle_device_bytes(fs_renderer *r);
uint64_t fs_release_idle_device_memory(int device);

uint32_t fs_get_width(const fs_renderer *r);
uint32_t fs_get_height(const fs_renderer *r);

/* ---- Multi-GPU: one frame row-tiled over the GPUs of one node, gathered over xGMI with RCCL (this project's addition;
 * the reference is single-device, GPU_Render.cu:113).  A group = one fs_renderer per device inside ONE process (the C++
 * drop-in of INTEGRATION.md is one process), RCCL communicators from ncclCommInitAll.  Rank r renders the 8-row bands
 * k*N + r (24-row bands for antialiasing 3) with the global-row delta-c mapping of fs_set_row_bands; slices are sent to
 * device 0 with ncclSend / ncclRecv in one ncclGroup on the members' compute streams, one kernel restores row order.
 * transport: 0 = RCCL (resolved with dlopen at first use; falls back to 1 with a message on stderr if unavailable; on hosts that only
 * support dmabuf IPC -- this pool -- HSA_ENABLE_IPC_MODE_LEGACY=0 must be in the environment before the process's FIRST HIP call: the
 * library sets it when it is loaded unless the host chose a value, so load it before anything touches HIP, or export the variable),
 * 1 = hipMemcpyPeerAsync (also chosen automatically when members share a device, e.g. tests on a one-GPU box).
 * Every fs_group_* upload / render call is the fs_* call of the same name applied to every member; renders are
 * asynchronous.  fs_group_render_current = gather + row reassembly + min / max / sum + D2H of the padded iteration buffer
 * (same layout as fs_render_current of a single renderer on the whole frame), asynchronous on member 0's compute stream;
 * fs_group_sync waits for everything.  Colours of the whole frame: fs_group_render_current_colors. */
typedef struct fs_group fs_group;
fs_group *fs_group_create(const int *devices, int n_devices, int transport);
void fs_group_destroy(fs_group *g);
int fs_group_size(const fs_group *g);
int fs_group_transport(const fs_group *g);
fs_renderer *fs_group_renderer(fs_group *g, int rank);
uint32_t fs_group_init_memory(fs_group *g, uint32_t w, uint32_t h, uint32_t antialiasing, uint32_t iter_bytes,
                              const fs_color16 *pal_interleaved, uint32_t pal_iters, uint32_t palette_aux_depth,
                              uint64_t palette_generation);
uint32_t fs_group_upload_orbit(fs_group *g, uint64_t generation, int type_tag, uint32_t iter_bytes, const void *entries,
                               uint64_t orbit_size, uint64_t uncompressed_size, uint64_t period_maybe_zero);
uint32_t fs_group_upload_orbit_compressed(fs_group *g, uint64_t generation, int type_tag, uint32_t iter_bytes,
                                          const void *entries, uint64_t compressed_size, uint64_t uncompressed_size,
                                          uint64_t period_maybe_zero, const void *orbit_x_low, const void *orbit_y_low);
uint32_t fs_group_upload_la(fs_group *g, uint64_t generation, int type_tag, uint32_t iter_bytes, const void *las,
                            uint32_t n_las, const void *stages, uint32_t n_stages, int is_valid, int use_at,
                            const void *at_info);
uint32_t fs_group_upload_bla(fs_group *g, int type_tag, const void *const *levels, const uint64_t *level_sizes,
                             int32_t n_levels, int32_t lm2);
uint32_t fs_group_upload_orbit_scaled(fs_group *g, int type_tag, uint32_t iter_bytes, const void *entries_t,
                                      const void *entries_f32, uint64_t orbit_size, uint64_t period_maybe_zero);
uint32_t fs_group_render_lav2(fs_group *g, int type_tag, int mode, int parity, const void *coords, uint64_t n_iterations);
uint32_t fs_group_render_bla(fs_group *g, int type_tag, const void *coords, uint64_t n_iterations);
uint32_t fs_group_render_scaled(fs_group *g, int type_tag, const void *coords, uint64_t n_iterations);
uint32_t fs_group_render_direct(fs_group *g, int type_tag, const void *coords, uint64_t n_iterations);
uint32_t fs_group_clear(fs_group *g);
uint32_t fs_group_render_current(fs_group *g, uint64_t n_iterations, void *iter_buffer, fs_reduction *reduction);
/* GPURenderer::RenderCurrent<IterType>(n, iters, colors, reduction, progressive) (GPU_Render.cu:556-581) for the group: as
 * fs_group_render_current, plus the Color16 buffer of the whole frame (antialias + palette on device 0 behind the row order,
 * N_color_cu = fs_color_buffer_elements(fs_group_renderer(g, 0)) elements, same layout as fs_render_current's).  Any of the
 * three host pointers may be NULL.  progressive != 0: a SNAPSHOT of the frame while the members' kernels are still writing it
 * -- nothing waits for a kernel; the slices are copied as they are on the members' display streams into buffers of their own
 * (it does not take part in the two-set rotation and does not count for fs_group_wait_current); fs_group_sync_display waits
 * for it. */
uint32_t fs_group_render_current_colors(fs_group *g, uint64_t n_iterations, void *iter_buffer, fs_color16 *color_buffer,
                                        fs_reduction *reduction, int progressive);
/* Where the iteration buffer of fs_group_render_current[_colors] travels (round 6).  0 (default) = gather: the slices go to device 0
 * over xGMI, one kernel restores row order, ONE copy brings the whole frame to the host over device 0's PCIe link.  1 = direct: every
 * member copies its own bands straight to their rows of iter_buffer over ITS OWN link (fs_copy_bands_to_host, on a copy stream of its
 * own behind its kernel, while it renders the next frame into its second slice) -- N links instead of one, no re-order kernel; the
 * gather then only runs when color_buffer or reduction is asked for (they need the frame on one device), and the frame itself no
 * longer crosses device 0's link.  iter_buffer should be page-locked and portable (hipHostMalloc(hipHostMallocPortable) /
 * fs_host_register).  Same frames either way (tests/test_gpu_group.py). */
uint32_t fs_group_set_host_path(fs_group *g, int host_path);
int fs_group_host_path(const fs_group *g);
uint32_t fs_group_sync_display(fs_group *g);
uint32_t fs_group_sync(fs_group *g);
/* Two frames may be in flight: fs_group_render_current runs on a stream of its own on device 0 (receive, row order,
 * reduction, D2H) behind the members' kernels, over one of TWO sets of gather / frame buffers used in rotation, so the
 * members' next frame can be launched right away and renders while this one is delivered.  fs_group_wait_current: the host
 * waits until the fs_group_render_current issued `frames_back` calls ago (0 = the latest, 1 = the one before) has filled
 * the caller's buffers -- the pipelined loop is  render k; render_current k (host buffer k % 2); wait_current(1).
 * The caller owns the host buffers: one per frame in flight.  (After fs_group_render_current member 0's own iteration
 * buffer is the OTHER set's slot: per-renderer colour output of a frame is taken before that call.) */
uint32_t fs_group_wait_current(fs_group *g, uint32_t frames_back);
/* The tiler's plan as a pure host function (tests; equals fractalshark_amd/tiling.py): rows rank `rank` owns, the
 * common padded slice height, and frame_index[y] = row of the gathered buffer (N slices back to back) that holds frame
 * row y.  Any output pointer may be NULL. */
void fs_group_plan(uint32_t height, uint32_t world, uint32_t band, uint32_t rank, uint32_t *local_rows,
                   uint32_t *max_local_rows, uint32_t *frame_index);

#ifdef __cplusplus
}
#endif

#endif /* FSMI355_H */
