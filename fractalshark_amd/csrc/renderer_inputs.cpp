// renderer_inputs.cpp -- what a frame is rendered from: the reference orbit, the LA table and the BLA table of a renderer
// (upload, device-side preparation, read-back), cached by generation number (GPU_Render.cu:440-487).
#include "renderer_state.hpp"

#include <cstddef>

using namespace fsr;

namespace {

// float4 units of the tuned loops' companion arrays of an n-entry HDRFloat<float> orbit (make_quiet_orbit lays them out;
// fs_orbit_device_bytes reports them)
constexpr uint64_t kQuietSlack = 32;
constexpr uint64_t quiet_orbit_units(uint64_t n)
{
    return 2 * (n + 2) + 16 + ((n + 2) + kQuietSlack + 1) / 2 + ((n + 2) + kQuietSlack) + ((n + 2) + kQuietSlack + 1) / 2;
}

// zq: the tuned LAv2 loop's view of the prepared orbit (same length incl. the two spare entries)
hipError_t make_quiet_orbit(fs_renderer *r, uint64_t n)
{
    (void)r_release(r, r->zq);
    // two companions back to back; the scaled runs request their entries one 8-entry body ahead, so the second one may be
    // read up to 16 entries past its end (never used)
    // ... followed by the compact form the 16-step body of the untested loop reads: 2Z alone (8 B per entry) and, per entry, the
    // block bounds of the entries 3, 7, 11 and 15 further on (16 B); 32 entries of slack each (the body after the last is
    // requested ahead, never used)
    // ... and the NDZ body bounds of FS_FAST_LOOP_FDU (two floats per entry), with the same slack
    const uint64_t m = n + 2, slack = kQuietSlack;
    const uint64_t units = quiet_orbit_units(n);
    hipError_t err = r_alloc(r, (void **)&r->zq, units * sizeof(float4), kInput);
    if (err != hipSuccess)
        return err;
    r->zq_n = m;
    r->zs2 = (float2 *)(r->zq + 2 * m + 16);
    r->zqb = r->zq + 2 * m + 16 + (m + slack + 1) / 2;
    r->znz = (float2 *)(r->zqb + (m + slack));
    err = hipMemsetAsync(r->zs2, 0, ((m + slack + 1) / 2 + (m + slack)) * sizeof(float4), r->compute);
    if (err != hipSuccess)
        return err;
    fsk_make_quiet_orbit(r->zref, r->zq, r->zs2, r->zqb, r->znz, m, r->compute);
    return hipGetLastError();
}

// The BLA table lives in ONE allocation: 64 level pointers (the device-side pointer table the kernels index by level), then
// the levels back to back, each 256-byte aligned; kept and reused when the next table fits (the reference re-allocates
// and re-uploads every level on every BLA render, GPU_Render.cu:1464-1479).
constexpr size_t kBlaPtrTableBytes = 64 * sizeof(void *);

void bla_release(fs_renderer *r)
{
    buf_release(r, r->bla_native);
    buf_release(r, r->bla_heap);
    buf_release(r, r->bla_block);
    r->bla_native_ok = r->bla_heap_ok = false;
    r->bla_level_mem.clear();
    r->bla_level_sizes.clear();
    r->bla_levels_dev = nullptr;
    r->bla_n_levels = 0;
}

// Lays out n_levels levels of sizes[l] records of rec_bytes in the block (growing it if needed) and uploads the pointer
// table on the compute stream.  A level of size 0 gets a NULL pointer.
hipError_t bla_layout(fs_renderer *r, const uint64_t *sizes, int32_t n_levels, size_t rec_bytes)
{
    if (n_levels > 64)
        return hipErrorInvalidValue;
    size_t total = kBlaPtrTableBytes;
    for (int32_t l = 0; l < n_levels; l++)
        total += (sizes[l] * rec_bytes + 255u) & ~(size_t)255u;
    r->bla_n_levels = 0;
    if (!r->bla_block.p || r->bla_block.cap < total) {
        bla_release(r); // (the native forms were made from the table that goes)
        const hipError_t e = buf_reserve(r, r->bla_block, total, kInput);
        if (e != hipSuccess)
            return e;
    }
    r->bla_level_mem.assign((size_t)n_levels, nullptr);
    r->bla_level_sizes.assign((size_t)n_levels, 0);
    size_t at = kBlaPtrTableBytes;
    for (int32_t l = 0; l < n_levels; l++) {
        if (sizes[l] == 0)
            continue;
        r->bla_level_mem[(size_t)l] = r->bla_block.as<char>() + at;
        r->bla_level_sizes[(size_t)l] = sizes[l];
        at += (sizes[l] * rec_bytes + 255u) & ~(size_t)255u;
    }
    r->bla_levels_dev = (const void **)r->bla_block.p;
    return hipMemcpyAsync(r->bla_block.p, r->bla_level_mem.data(), sizeof(void *) * (size_t)n_levels, hipMemcpyHostToDevice,
                          r->compute);
}

// A new orbit is in place: the native BLA table carries arrival entries of the previous one.
void orbit_changed(fs_renderer *r)
{
    r->bla_native_ok = false;
    r->bla_native_stale = r->bla_n_levels > 0 && r->bla_type == FS_T_HDR32;
}

// The compressed-resident form of the orbit (runtime decompression) goes whenever another orbit is about to come in.
void drop_seq(fs_renderer *r)
{
    (void)r_release(r, r->wp_raw);
    r->orbit_seq = false;
}

} // namespace

namespace fsr {

// The installed LA table (records + stages): the buffers of the previous table are kept when the new one fits.
hipError_t la_reserve(fs_renderer *r, size_t las_bytes, size_t stages_bytes)
{
    const hipError_t e = buf_reserve(r, r->las, las_bytes, kInput);
    return e != hipSuccess ? e : buf_reserve(r, r->stages, stages_bytes, kInput);
}

// Device-native form of the HDRFloat<float> table just installed in the block (see FsBlaRec, kernels.h).  Leaves
// bla_native_ok = false -- the kernels then read the reference-layout records -- when the table has more than
// kBlaMaxLevels levels or 2^32 records, when memory for it cannot be had, or when an r2 is not a reduced non-negative finite
// value (the integer-key compare would then differ from the reference's float compare).  Synchronises the compute stream.
uint32_t bla_make_native(fs_renderer *r, int32_t n_levels)
{
    r->bla_native_ok = false;
    r->bla_native_stale = false;
    if (n_levels <= 2 || n_levels > kBlaMaxLevels || r->bla_type != FS_T_HDR32 || !r->orbit_ok ||
        r->orbit_type != FS_T_HDR32 || !r->zref)
        return 0;
    uint64_t total = 0;
    for (int32_t l = 2; l < n_levels; l++) {
        r->bla_level_off[l] = (uint32_t)total;
        total += r->bla_level_sizes[(size_t)l];
    }
    if (total == 0 || total > 0xFFFFFFF0ull)
        return 0;
    // (+ the lookup's pre-test keys, one per orbit index 4 q + 1)
    const uint32_t n_kmax = (uint32_t)(r->orbit_uncompressed / 4u) + 2u;
    const size_t need = 256 + (size_t)total * (sizeof(FsBlaRec) + 2 * sizeof(int4)) + (size_t)n_kmax * sizeof(long long);
    if (buf_reserve(r, r->bla_native, need, kInput) != hipSuccess) {
        (void)hipGetLastError();
        return 0; // not an error: the reference-layout table serves
    }
    uint32_t *bad = r->bla_native.as<uint32_t>();
    FsBlaRec *rec = (FsBlaRec *)(r->bla_native.as<char>() + 256);
    int4 *lad = (int4 *)((char *)rec + (size_t)total * sizeof(FsBlaRec));
    FS_TRY(hipMemsetAsync(bad, 0, 256, r->compute));
    fsk_bla_make_native((const fs_bla_hdr32 *const *)r->bla_levels_dev, r->bla_level_off, r->bla_level_sizes.data(), n_levels,
                        r->zref, (uint32_t)r->orbit_uncompressed, rec, lad, bad, r->bla_lm2,
                        (long long *)(lad + 2 * (size_t)total), n_kmax, r->compute);
    FS_TRY(hipGetLastError());
    uint32_t flag = 1;
    FS_TRY(hipMemcpyAsync(&flag, bad, 4, hipMemcpyDeviceToHost, r->compute));
    FS_TRY(hipStreamSynchronize(r->compute));
    r->bla_native_total = (uint32_t)total;
    r->bla_native_ok = flag == 0;
    // ... and its heap-numbered copy for the hand-written kernel (not an error when it cannot be had: the compiled kernel serves)
    r->bla_heap_ok = false;
    const uint64_t hn = fsk_bla_heap_positions(r->bla_level_sizes.data(), n_levels);
    // (orbit positions below 2^24: the kernel forms the address of Q[(m - 1) / 4] with one 24-bit multiply-add)
    if (r->bla_native_ok && hn != 0 && r->orbit_uncompressed < 0x00FFFFF0ull) {
        const size_t nz = (size_t)r->orbit_uncompressed + 2u;
        const size_t hneed = (size_t)hn * (sizeof(FsBlaRec) + 2 * sizeof(int4)) + (size_t)n_kmax * 3 * sizeof(int4) + nz * sizeof(float4);
        if (buf_reserve(r, r->bla_heap, hneed, kInput) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
        FS_TRY(hipMemsetAsync(r->bla_heap.p, 0, hneed, r->compute));
        FsBlaRec *hrec = r->bla_heap.as<FsBlaRec>();
        int4 *hlad = (int4 *)(hrec + hn);
        int4 *hq = hlad + 2 * (size_t)hn;
        float4 *zb = (float4 *)(hq + 3 * (size_t)n_kmax);
        fsk_bla_make_heap(rec, lad, (const long long *)(lad + 2 * (size_t)total), n_kmax, r->bla_level_off,
                          r->bla_level_sizes.data(), n_levels, r->bla_lm2, r->zref, (uint32_t)r->orbit_uncompressed, hrec, hlad, hq,
                          zb, r->compute);
        FS_TRY(hipGetLastError());
        FS_TRY(hipStreamSynchronize(r->compute));
        r->bla_heap_positions = hn;
        r->bla_heap_nq = n_kmax;
        r->bla_heap_ok = true;
    }
    return 0;
}

void free_perturb(fs_renderer *r)
{
    (void)r_release(r, r->zref);
    (void)r_release(r, r->zq);
    (void)r_release(r, r->zref64);
    drop_seq(r);
    (void)r_release(r, r->orbit_f64);
    (void)r_release(r, r->orbit_plain);
    (void)r_release(r, r->orbit_2x32);
    (void)r_release(r, r->scaled_t);
    (void)r_release(r, r->scaled_f);
    r->scaled_count = 0;
    r->orbit_ok = false;
    r->orbit_gen = 0;
    buf_release(r, r->las);
    buf_release(r, r->stages);
    r->la_ok = false;
    r->la_gen = 0;
    bla_release(r);
}

} // namespace fsr

// uint64_t IterType tables (fs_la_*_u64 / fs_la_stage_u64 / fs_at_*_u64) are narrowed to the uint32_t device records.
template <class R64, class R32> static bool narrow_la(const void *in, uint32_t n, std::vector<uint8_t> &out)
{
    out.resize((size_t)n * sizeof(R32));
    const R64 *src = (const R64 *)in;
    R32 *dst = (R32 *)out.data();
    for (uint32_t i = 0; i < n; i++) {
        if (src[i].StepLength > 0xFFFFFFFFull || src[i].NextStageLAIndex > 0xFFFFFFFFull)
            return false;
        memcpy(&dst[i], &src[i], offsetof(R32, StepLength)); // Ref .. MinMag are laid out identically
        dst[i].StepLength = (uint32_t)src[i].StepLength;
        dst[i].NextStageLAIndex = (uint32_t)src[i].NextStageLAIndex;
    }
    return true;
}

// FNV-1a over the size, the period and up to 4096 evenly spread 8-byte words of an orbit's entries (never 0)
static uint64_t orbit_fingerprint(const void *entries, uint64_t bytes, uint64_t size, uint64_t period, int type_tag)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](uint64_t v) {
        for (int i = 0; i < 8; i++) {
            h ^= (v >> (8 * i)) & 0xFFu;
            h *= 1099511628211ull;
        }
    };
    mix(size), mix(period), mix((uint64_t)type_tag);
    const uint64_t words = bytes / 8u;
    const uint64_t stride = words > 4096u ? words / 4096u : 1u;
    const unsigned char *p = (const unsigned char *)entries;
    for (uint64_t w = 0; w < words; w += stride) {
        uint64_t v;
        memcpy(&v, p + w * 8u, 8);
        mix(v);
    }
    if (words != 0u) { // the last word, whatever the stride
        uint64_t v;
        memcpy(&v, p + (words - 1u) * 8u, 8);
        mix(v);
    }
    return h != 0ull ? h : 1ull;
}

// The slot of an orbit that the kernels read in the layout of the upload (plain float / CudaDblflt, double,
// HDRFloat<CudaDblflt>) and the size of its records.
static void **as_uploaded_slot(fs_renderer *r, int type_tag, size_t *rec_bytes)
{
    switch (type_tag) {
    case FS_T_F32: // GPUReferenceIter<float,Disable> (8 B)
        *rec_bytes = sizeof(fs_orbit_f32);
        return &r->orbit_plain;
    case FS_T_2X32: // GPUReferenceIter<CudaDblflt,Disable> (16 B)
        *rec_bytes = sizeof(fs_orbit_p2x32);
        return &r->orbit_plain;
    case FS_T_F64:
        *rec_bytes = sizeof(fs_orbit_f64);
        return (void **)&r->orbit_f64;
    default:
        *rec_bytes = sizeof(fs_orbit_2x32);
        return (void **)&r->orbit_2x32;
    }
}

// Another orbit of this type is about to come in: the slot of ITS type is freed (an orbit of another type stays allocated
// until free_perturb), and nothing is resident until install_orbit.
static uint32_t retire_orbit(fs_renderer *r, int type_tag)
{
    if (type_tag == FS_T_HDR32 || type_tag == FS_T_HDR64) {
        FS_TRY(r_release(r, r->zref));
        FS_TRY(r_release(r, r->zref64));
    } else {
        size_t rec_bytes;
        FS_TRY(r_release(r, *as_uploaded_slot(r, type_tag, &rec_bytes)));
    }
    r->orbit_ok = false;
    drop_seq(r);
    return 0;
}

// An upload has replaced the resident orbit.  `seq`: only its waypoints are resident (wp_raw).
static void install_orbit(fs_renderer *r, uint64_t generation, int type_tag, uint64_t size, uint64_t uncompressed_size,
                          uint64_t period_maybe_zero, bool seq = false)
{
    r->orbit_seq = seq;
    r->orbit_size = size;
    r->orbit_uncompressed = uncompressed_size;
    r->orbit_period = period_maybe_zero;
    r->orbit_gen = generation;
    if (r->pending_fp == 0ull || r->pending_fp != r->orbit_fp)
        r->orbit_epoch++;
    r->orbit_fp = r->pending_fp;
    r->pending_fp = 0ull;
    r->orbit_type = type_tag;
    r->orbit_ok = true;
    orbit_changed(r);
}

extern "C" {

uint32_t fs_upload_orbit(fs_renderer *r, uint64_t generation, int type_tag, uint32_t iter_bytes, const void *entries,
                         uint64_t orbit_size, uint64_t uncompressed_size, uint64_t period_maybe_zero)
{
    if (uint32_t e = use_device(r))
        return e;
    // orbit entries do not depend on IterType (GPU_ReferenceIter.h:52-127); counts must fit the 32-bit device counters
    if ((type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64 && type_tag != FS_T_F64 && type_tag != FS_T_HDR2X32 &&
         type_tag != FS_T_F32 && type_tag != FS_T_2X32) ||
        (iter_bytes != 4 && iter_bytes != 8) || uncompressed_size > 0xFFFFFFFFull)
        return FS_ERR_UNSUPPORTED;
    if (!r->compute)
        return FS_ERR_6;
    if (r->orbit_ok && r->orbit_gen == generation && generation != 0 && r->orbit_type == type_tag)
        return 0; // cached by generation number (GPU_Render.cu:440-487)
    if (uint32_t e = retire_orbit(r, type_tag))
        return e;
    if (type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64) {
        // used as uploaded; the plain types get one spare record
        size_t eb;
        void **slot = as_uploaded_slot(r, type_tag, &eb);
        const uint64_t spare = (type_tag == FS_T_F32 || type_tag == FS_T_2X32) ? 1u : 0u;
        FS_TRY(r_alloc(r, slot, (orbit_size + spare) * eb, kInput));
        FS_TRY(hipMemcpyAsync(*slot, entries, orbit_size * eb, hipMemcpyDefault, r->compute));
        FS_TRY(hipStreamSynchronize(r->compute));
        install_orbit(r, generation, type_tag, orbit_size, uncompressed_size, period_maybe_zero);
        return 0;
    }
    const size_t in_bytes = type_tag == FS_T_HDR32 ? sizeof(fs_orbit_hdr32) : sizeof(fs_orbit_hdr64);
    r->pending_fp = orbit_fingerprint(entries, orbit_size * in_bytes, orbit_size, period_maybe_zero, type_tag);
    void *raw = nullptr;
    FS_TRY(r_alloc(r, &raw, orbit_size * in_bytes, kInput));
    // two spare entries: the tuned loops may prefetch one entry past the end
    hipError_t err = type_tag == FS_T_HDR32 ? r_alloc(r, (void **)&r->zref, (orbit_size + 2) * sizeof(float4), kInput)
                                            : r_alloc(r, (void **)&r->zref64, (orbit_size + 2) * sizeof(FsZ64), kInput);
    if (err == hipSuccess)
        err = hipMemcpyAsync(raw, entries, orbit_size * in_bytes, hipMemcpyDefault, r->compute);
    if (err == hipSuccess) {
        if (type_tag == FS_T_HDR32) {
            err = hipMemsetAsync(r->zref + orbit_size, 0, 2 * sizeof(float4), r->compute);
            fsk_prepare_orbit_hdr32((const fs_orbit_hdr32 *)raw, r->zref, orbit_size, r->compute);
            if (err == hipSuccess)
                err = make_quiet_orbit(r, orbit_size);
        } else {
            err = hipMemsetAsync(r->zref64 + orbit_size, 0, 2 * sizeof(FsZ64), r->compute);
            fsk_prepare_orbit_hdr64((const fs_orbit_hdr64 *)raw, r->zref64, orbit_size, r->compute);
        }
        if (err == hipSuccess)
            err = hipGetLastError();
    }
    if (err == hipSuccess)
        err = hipStreamSynchronize(r->compute);
    (void)r_free(r, raw);
    if (err != hipSuccess)
        return (uint32_t)err;
    install_orbit(r, generation, type_tag, orbit_size, uncompressed_size, period_maybe_zero);
    return 0;
}

uint32_t fs_upload_orbit_compressed(fs_renderer *r, uint64_t generation, int type_tag, uint32_t iter_bytes,
                                    const void *entries, uint64_t compressed_size, uint64_t uncompressed_size,
                                    uint64_t period_maybe_zero, const void *orbit_x_low, const void *orbit_y_low)
{
    if (uint32_t e = use_device(r))
        return e;
    if ((type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64 && type_tag != FS_T_F32 && type_tag != FS_T_F64 &&
         type_tag != FS_T_2X32 && type_tag != FS_T_HDR2X32) ||
        (iter_bytes != 4 && iter_bytes != 8) || !orbit_x_low || !orbit_y_low)
        return FS_ERR_UNSUPPORTED;
    if (!r->compute)
        return FS_ERR_6;
    const bool want_seq = r->compressed_mode == 1;
    // an EXPANDED orbit must fit the 32-bit positions of the kernels that read it (and the device: 2^32 entries are 64 GiB
    // and more); a waypoint-resident one may be any length -- its positions are 64-bit in the kernel that walks it
    if (!want_seq && uncompressed_size > 0xFFFFFFFFull)
        return FS_ERR_UNSUPPORTED; // (fs_set_compressed_orbit_mode(1) serves such an orbit)
    if (r->orbit_ok && r->orbit_gen == generation && generation != 0 && r->orbit_type == type_tag && r->orbit_seq == want_seq)
        return 0;
    if (uint32_t e = retire_orbit(r, type_tag))
        return e;
    if (type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64) {
        // float / double / CudaDblflt / HDRFloat<CudaDblflt>: expanded into the record array the uncompressed upload
        // of that type fills (kernels_decompress.hip)
        size_t out_b;
        void **slot = as_uploaded_slot(r, type_tag, &out_b);
        const size_t in_b = type_tag == FS_T_F32    ? sizeof(fs_orbit_f32_rc)
                            : type_tag == FS_T_2X32 ? sizeof(fs_orbit_p2x32_rc)
                            : type_tag == FS_T_F64  ? sizeof(fs_orbit_f64_rc)
                                                    : sizeof(fs_orbit_2x32_rc);
        if (want_seq) {
            // keep the waypoints, nothing else: k_lav2_plain / k_lav2_2x32 walk them with a cursor per pixel (same values as
            // the expansion below, entry for entry)
            if (compressed_size == 0 || compressed_size > 0xFFFFFFFFull || uncompressed_size > 0xFFFFFFFFull)
                return FS_ERR_UNSUPPORTED; // (these kernels keep 32-bit positions)
            const size_t low_b = type_tag == FS_T_F32 ? sizeof(float) : (type_tag == FS_T_HDR2X32 ? sizeof(fs_real_2x32) : 8u);
            FS_TRY(r_alloc(r, &r->wp_raw, compressed_size * in_b, kInput));
            FS_TRY(hipMemcpyAsync(r->wp_raw, entries, compressed_size * in_b, hipMemcpyDefault, r->compute));
            FS_TRY(hipStreamSynchronize(r->compute));
            memset(r->c_low_plain, 0, sizeof(r->c_low_plain));
            memcpy(r->c_low_plain[0], orbit_x_low, low_b);
            memcpy(r->c_low_plain[1], orbit_y_low, low_b);
            install_orbit(r, generation, type_tag, compressed_size, uncompressed_size, period_maybe_zero, true);
            return 0;
        }
        void *raw = nullptr;
        FS_TRY(r_alloc(r, &raw, compressed_size * in_b, kInput));
        hipError_t err = r_alloc(r, slot, (uncompressed_size + 1) * out_b, kInput);
        if (err == hipSuccess)
            err = hipMemcpyAsync(raw, entries, compressed_size * in_b, hipMemcpyDefault, r->compute);
        if (err == hipSuccess)
            err = hipMemsetAsync((char *)*slot + uncompressed_size * out_b, 0, out_b, r->compute);
        if (err == hipSuccess) {
            fsk_decompress_orbit_plain(type_tag, raw, compressed_size, uncompressed_size, orbit_x_low, orbit_y_low, *slot,
                                       r->compute);
            err = hipGetLastError();
        }
        if (err == hipSuccess)
            err = hipStreamSynchronize(r->compute);
        (void)r_free(r, raw);
        if (err != hipSuccess)
            return (uint32_t)err;
        install_orbit(r, generation, type_tag, compressed_size, uncompressed_size, period_maybe_zero);
        return 0;
    }
    const size_t in_bytes = type_tag == FS_T_HDR32 ? sizeof(fs_orbit_hdr32_rc) : sizeof(fs_orbit_hdr64_rc);
    if (want_seq) {
        // keep the waypoints, nothing else: the kernel decompresses as it goes (GPUPerturbSingleResults for
        // PerturbExtras::SimpleCompression uploads exactly this array, Perturb.cuh:51-80)
        if (compressed_size == 0 || compressed_size > 0xFFFFFFFFull)
            return FS_ERR_UNSUPPORTED;
        FS_TRY(r_alloc(r, &r->wp_raw, compressed_size * in_bytes, kInput));
        FS_TRY(hipMemcpyAsync(r->wp_raw, entries, compressed_size * in_bytes, hipMemcpyDefault, r->compute));
        FS_TRY(hipStreamSynchronize(r->compute));
        if (type_tag == FS_T_HDR32) {
            r->c_low32[0] = *(const fs_real_hdr32 *)orbit_x_low;
            r->c_low32[1] = *(const fs_real_hdr32 *)orbit_y_low;
        } else {
            r->c_low64[0] = *(const fs_real_hdr64 *)orbit_x_low;
            r->c_low64[1] = *(const fs_real_hdr64 *)orbit_y_low;
        }
        install_orbit(r, generation, type_tag, compressed_size, uncompressed_size, period_maybe_zero, true);
        return 0;
    }
    void *raw = nullptr;
    FS_TRY(r_alloc(r, &raw, compressed_size * in_bytes, kInput));
    hipError_t err = type_tag == FS_T_HDR32 ? r_alloc(r, (void **)&r->zref, (uncompressed_size + 2) * sizeof(float4), kInput)
                                            : r_alloc(r, (void **)&r->zref64, (uncompressed_size + 2) * sizeof(FsZ64), kInput);
    if (err == hipSuccess)
        err = hipMemcpyAsync(raw, entries, compressed_size * in_bytes, hipMemcpyDefault, r->compute);
    if (err == hipSuccess) {
        if (type_tag == FS_T_HDR32) {
            err = hipMemsetAsync(r->zref + uncompressed_size, 0, 2 * sizeof(float4), r->compute);
            fsk_decompress_orbit_hdr32((const fs_orbit_hdr32_rc *)raw, compressed_size, uncompressed_size,
                                       *(const fs_real_hdr32 *)orbit_x_low, *(const fs_real_hdr32 *)orbit_y_low, r->zref,
                                       r->compute);
            if (err == hipSuccess)
                err = make_quiet_orbit(r, uncompressed_size);
        } else {
            err = hipMemsetAsync(r->zref64 + uncompressed_size, 0, 2 * sizeof(FsZ64), r->compute);
            fsk_decompress_orbit_hdr64((const fs_orbit_hdr64_rc *)raw, compressed_size, uncompressed_size,
                                       *(const fs_real_hdr64 *)orbit_x_low, *(const fs_real_hdr64 *)orbit_y_low, r->zref64,
                                       r->compute);
        }
        if (err == hipSuccess)
            err = hipGetLastError();
    }
    if (err == hipSuccess)
        err = hipStreamSynchronize(r->compute);
    (void)r_free(r, raw);
    if (err != hipSuccess)
        return (uint32_t)err;
    install_orbit(r, generation, type_tag, compressed_size, uncompressed_size, period_maybe_zero);
    return 0;
}

uint32_t fs_upload_orbit_scaled(fs_renderer *r, int type_tag, uint32_t iter_bytes, const void *entries_t,
                                const void *entries_f32, uint64_t orbit_size, uint64_t period_maybe_zero)
{
    (void)period_maybe_zero;
    if (uint32_t e = use_device(r))
        return e;
    if ((type_tag != FS_T_HDR32 && type_tag != FS_T_F64) || (iter_bytes != 4 && iter_bytes != 8) ||
        orbit_size > 0xFFFFFFFFull || orbit_size < 2)
        return FS_ERR_UNSUPPORTED;
    if (!r->compute)
        return FS_ERR_6;
    FS_TRY(r_release(r, r->scaled_t));
    FS_TRY(r_release(r, r->scaled_f));
    r->scaled_count = 0;
    const size_t t_bytes = type_tag == FS_T_HDR32 ? sizeof(fs_orbit_hdr32_bad) : sizeof(fs_orbit_f64_bad);
    FS_TRY(r_alloc(r, &r->scaled_t, orbit_size * t_bytes, kInput));
    // (the tuned kernel requests its binary32 entries four steps ahead: up to three entries past the end are read, never used)
    FS_TRY(r_alloc(r, (void **)&r->scaled_f, (orbit_size + 8) * sizeof(fs_orbit_f32_bad), kInput));
    FS_TRY(hipMemsetAsync(r->scaled_f + orbit_size, 0, 8 * sizeof(fs_orbit_f32_bad), r->compute));
    FS_TRY(hipMemcpyAsync(r->scaled_t, entries_t, orbit_size * t_bytes, hipMemcpyDefault, r->compute));
    FS_TRY(hipMemcpyAsync(r->scaled_f, entries_f32, orbit_size * sizeof(fs_orbit_f32_bad), hipMemcpyDefault, r->compute));
    fsk_scaled_bounds(r->scaled_f, orbit_size, r->compute); // the tuned kernel's per-entry bound, in the padding word
    FS_TRY(hipStreamSynchronize(r->compute)); // host buffers are borrowed for the call only
    r->scaled_count = orbit_size;
    r->scaled_type = type_tag;
    return 0;
}

uint32_t fs_upload_la(fs_renderer *r, uint64_t generation, int type_tag, uint32_t iter_bytes, const void *las,
                      uint32_t n_las, const void *stages, uint32_t n_stages, int is_valid, int use_at,
                      const void *at_info)
{
    if (uint32_t e = use_device(r))
        return e;
    const bool plain = type_tag == FS_T_F32 || type_tag == FS_T_F64 || type_tag == FS_T_2X32;
    if ((type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64 && type_tag != FS_T_HDR2X32 && !plain) ||
        (iter_bytes != 4 && iter_bytes != 8))
        return FS_ERR_UNSUPPORTED;
    if (!r->compute)
        return FS_ERR_6;
    if (r->la_ok && r->la_gen == generation && generation != 0 && r->la_type == type_tag)
        return 0;
    const size_t la_bytes = type_tag == FS_T_HDR32   ? sizeof(fs_la_hdr32_u32)
                            : type_tag == FS_T_HDR64 ? sizeof(fs_la_hdr64_u32)
                            : type_tag == FS_T_F32   ? sizeof(fs_la_f32_u32)
                            : type_tag == FS_T_F64   ? sizeof(fs_la_f64_u32)
                            : type_tag == FS_T_2X32  ? sizeof(fs_la_p2x32_u32)
                                                     : sizeof(fs_la_2x32_u32);
    // size of the uint32_t ATInfo record and the offset of its second field in the uint32_t / uint64_t records
    const size_t at_bytes = type_tag == FS_T_HDR32   ? sizeof(fs_at_hdr32_u32)
                            : type_tag == FS_T_HDR64 ? sizeof(fs_at_hdr64_u32)
                            : type_tag == FS_T_F32   ? sizeof(fs_at_f32_u32)
                            : type_tag == FS_T_F64   ? sizeof(fs_at_f64_u32)
                            : type_tag == FS_T_2X32  ? sizeof(fs_at_p2x32_u32)
                                                     : sizeof(fs_at_2x32_u32);
    const size_t at_rest32 = (type_tag == FS_T_HDR64 || type_tag == FS_T_F64) ? 8 : 4;
    std::vector<uint8_t> las32, stages32;
    uint8_t at32[sizeof(fs_at_hdr64_u32)] = {0};
    bool keep_u64 = false; // the LA records stay in the reference's uint64_t layout
    uint32_t at_step_hi = 0;
    size_t la_bytes_up = la_bytes;
    if (iter_bytes == 8) {
        bool ok = true;
        // HDRFloat<float | double> tables under fs_set_compressed_orbit_mode(1) are read by the waypoint-resident kernel,
        // whose wide instantiation takes the uint64_t records as they are: kept whenever a step length or index does not fit
        // 32 bits (an orbit of 2^32 and more uncompressed entries), and under the FS_VARIANT_WIDE_COUNTERS test switch
        const bool can_keep = (type_tag == FS_T_HDR32 || type_tag == FS_T_HDR64) && r->compressed_mode == 1;
        keep_u64 = can_keep && (r->variant & FS_VARIANT_FLAG_WIDE) != 0;
        if (n_las && !keep_u64) {
            ok = type_tag == FS_T_HDR32   ? narrow_la<fs_la_hdr32_u64, fs_la_hdr32_u32>(las, n_las, las32)
                 : type_tag == FS_T_HDR64 ? narrow_la<fs_la_hdr64_u64, fs_la_hdr64_u32>(las, n_las, las32)
                 : type_tag == FS_T_F32   ? narrow_la<fs_la_f32_u64, fs_la_f32_u32>(las, n_las, las32)
                 : type_tag == FS_T_F64   ? narrow_la<fs_la_f64_u64, fs_la_f64_u32>(las, n_las, las32)
                 : type_tag == FS_T_2X32  ? narrow_la<fs_la_p2x32_u64, fs_la_p2x32_u32>(las, n_las, las32)
                                          : narrow_la<fs_la_2x32_u64, fs_la_2x32_u32>(las, n_las, las32);
            if (!ok && can_keep)
                keep_u64 = ok = true;
        }
        stages32.resize((size_t)n_stages * sizeof(fs_la_stage_u32));
        for (uint32_t i = 0; ok && i < n_stages; i++) {
            // (a stage's first record and its record count index the table itself, whose size is a uint32_t)
            const fs_la_stage_u64 &sg = ((const fs_la_stage_u64 *)stages)[i];
            if (sg.LAIndex > 0xFFFFFFFFull || sg.MacroItCount > 0xFFFFFFFFull)
                return (uint32_t)hipErrorInvalidValue;
            ((fs_la_stage_u32 *)stages32.data())[i] = fs_la_stage_u32{(uint32_t)sg.LAIndex, (uint32_t)sg.MacroItCount};
        }
        if (ok && at_info) {
            uint64_t step;
            memcpy(&step, at_info, 8);
            if (keep_u64)
                at_step_hi = (uint32_t)(step >> 32);
            else
                ok = step <= 0xFFFFFFFFull;
            const uint32_t step32 = (uint32_t)step;
            memcpy(at32, &step32, 4);
            // everything after StepLength is laid out identically; it starts at offset 8 in the uint64_t record
            memcpy(at32 + at_rest32, (const uint8_t *)at_info + 8, at_bytes - at_rest32);
            at_info = at32;
        }
        if (!ok)
            return FS_ERR_UNSUPPORTED; // a step length / index beyond 32 bits for a kernel that reads an EXPANDED orbit
        if (keep_u64)
            la_bytes_up = type_tag == FS_T_HDR32 ? sizeof(fs_la_hdr32_u64) : sizeof(fs_la_hdr64_u64);
        else
            las = las32.data();
        stages = stages32.data();
    }
    r->la_ok = false;
    FS_TRY(la_reserve(r, (size_t)n_las * la_bytes_up, (size_t)n_stages * sizeof(fs_la_stage_u32)));
    if (n_las)
        FS_TRY(hipMemcpyAsync(r->las.p, las, (size_t)n_las * la_bytes_up, hipMemcpyDefault, r->compute));
    r->la_u64 = keep_u64;
    r->at_step_hi = at_step_hi;
    if (n_stages)
        FS_TRY(hipMemcpyAsync(r->stages.p, stages, (size_t)n_stages * sizeof(fs_la_stage_u32), hipMemcpyDefault,
                              r->compute));
    FS_TRY(hipStreamSynchronize(r->compute));
    r->n_las = n_las;
    r->n_stages = n_stages;
    r->la_valid = is_valid;
    r->use_at = use_at;
    memset(&r->at, 0, sizeof(r->at));
    memset(&r->at64, 0, sizeof(r->at64));
    memset(&r->at2x32, 0, sizeof(r->at2x32));
    memset(r->at_plain, 0, sizeof(r->at_plain));
    if (at_info && plain)
        memcpy(r->at_plain, at_info, at_bytes);
    else if (at_info && type_tag == FS_T_HDR32)
        memcpy(&r->at, at_info, sizeof(r->at));
    else if (at_info && type_tag == FS_T_HDR2X32)
        memcpy(&r->at2x32, at_info, sizeof(r->at2x32));
    else if (at_info)
        memcpy(&r->at64, at_info, sizeof(r->at64));
    else
        r->use_at = 0;
    r->la_type = type_tag;
    r->la_gen = generation;
    r->la_ok = true;
    return 0;
}

uint32_t fs_upload_bla(fs_renderer *r, int type_tag, const void *const *levels, const uint64_t *level_sizes,
                       int32_t n_levels, int32_t lm2)
{
    if (uint32_t e = use_device(r))
        return e;
    if (type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64 && type_tag != FS_T_F64)
        return FS_ERR_UNSUPPORTED;
    if (!r->compute)
        return FS_ERR_6;
    const size_t rec_bytes = type_tag == FS_T_HDR32 ? sizeof(fs_bla_hdr32)
                                                    : (type_tag == FS_T_HDR64 ? sizeof(fs_bla_hdr64) : sizeof(fs_bla_f64));
    r->bla_type = type_tag;
    r->bla_n_levels = 0;
    if (n_levels <= 0)
        return 0;
    std::vector<uint64_t> sizes((size_t)n_levels, 0);
    for (int32_t l = 0; l < n_levels; l++)
        sizes[(size_t)l] = levels[l] ? level_sizes[l] : 0;
    FS_TRY(bla_layout(r, sizes.data(), n_levels, rec_bytes));
    for (int32_t l = 0; l < n_levels; l++)
        if (sizes[(size_t)l])
            FS_TRY(hipMemcpyAsync(r->bla_level_mem[(size_t)l], levels[l], sizes[(size_t)l] * rec_bytes, hipMemcpyDefault,
                                  r->compute));
    FS_TRY(hipStreamSynchronize(r->compute)); // the host levels are borrowed for the call only
    r->bla_n_levels = n_levels;
    r->bla_lm2 = lm2;
    r->bla_native_ok = false;
    r->bla_native_stale = type_tag == FS_T_HDR32; // made by the next BLA render: it also needs the orbit of that render
    return 0;
}

uint32_t fs_build_bla(fs_renderer *r, int type_tag, const void *bla_size)
{
    if (uint32_t e = use_device(r))
        return e;
    if (type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64)
        return FS_ERR_UNSUPPORTED;
    if (!r->compute || !r->orbit_ok || r->orbit_type != type_tag)
        return FS_ERR_6;
    if (r->orbit_seq)
        return FS_ERR_UNSUPPORTED; // needs the expanded orbit (fs_set_compressed_orbit_mode 0)
    const size_t rec_bytes = type_tag == FS_T_HDR32 ? sizeof(fs_bla_hdr32) : sizeof(fs_bla_hdr64);
    r->bla_n_levels = 0;
    r->bla_type = type_tag;
    // BLAS::Init, BLAS.cpp:218-241: elements per level halve (rounding up) from count-1 down to 1
    const uint64_t InM = r->orbit_uncompressed;
    uint64_t m = InM ? InM - 1 : 0;
    if (InM == 0 || m == 0)
        return 0;
    std::vector<uint64_t> epl;
    for (; m > 1; m = (m + 1) >> 1)
        epl.push_back(m);
    epl.push_back(m);
    const int n_levels = (int)epl.size();
    int32_t lm2 = n_levels - 2;
    if (lm2 < 0)
        lm2 = 0;
    std::vector<uint64_t> materialised(epl); // m_FirstLevel = 2: levels 0 and 1 get no memory (NULL pointers)
    materialised[0] = 0;
    if (n_levels > 1)
        materialised[1] = 0;
    FS_TRY(bla_layout(r, materialised.data(), n_levels, rec_bytes));
    const std::vector<void *> &ptrs = r->bla_level_mem;
    {
        TimedLaunch t(r);
        if (type_tag == FS_T_HDR32)
            fsk_bla_build_hdr32(r->zref, ptrs.data(), epl.data(), n_levels, *(const fs_real_hdr32 *)bla_size, r->compute);
        else
            fsk_bla_build_hdr64(r->zref64, ptrs.data(), epl.data(), n_levels, *(const fs_real_hdr64 *)bla_size, r->compute);
    }
    FS_TRY(hipGetLastError());
    FS_TRY(hipStreamSynchronize(r->compute)); // ptrs / epl are host temporaries of this call
    r->bla_n_levels = n_levels;
    r->bla_lm2 = lm2;
    r->bla_native_ok = false;
    r->bla_native_stale = type_tag == FS_T_HDR32; // made by the next BLA render: it also needs the orbit of that render
    return 0;
}

uint32_t fs_la_counts(const fs_renderer *r, uint32_t *n_las, uint32_t *n_stages, int *use_at, int *is_valid)
{
    if (!r->la_ok)
        return FS_ERR_6;
    if (n_las)
        *n_las = r->n_las;
    if (n_stages)
        *n_stages = r->n_stages;
    if (use_at)
        *use_at = r->use_at;
    if (is_valid)
        *is_valid = r->la_valid;
    return 0;
}

uint32_t fs_read_la(fs_renderer *r, void *las_out, uint32_t max_las, void *stages_out, uint32_t max_stages, void *at_out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->la_ok || (r->la_type != FS_T_HDR32 && r->la_type != FS_T_HDR64))
        return FS_ERR_6;
    const size_t rec_bytes = r->la_type == FS_T_HDR32 ? sizeof(fs_la_hdr32_u32) : sizeof(fs_la_hdr64_u32);
    const uint32_t nl = r->n_las < max_las ? r->n_las : max_las, ns = r->n_stages < max_stages ? r->n_stages : max_stages;
    if (las_out && nl)
        FS_TRY(hipMemcpyAsync(las_out, r->las.p, rec_bytes * nl, hipMemcpyDeviceToHost, r->compute));
    if (stages_out && ns)
        FS_TRY(hipMemcpyAsync(stages_out, r->stages.p, sizeof(fs_la_stage_u32) * ns, hipMemcpyDeviceToHost, r->compute));
    FS_TRY(hipStreamSynchronize(r->compute));
    if (at_out) {
        if (r->la_type == FS_T_HDR32)
            memcpy(at_out, &r->at, sizeof(r->at));
        else
            memcpy(at_out, &r->at64, sizeof(r->at64));
    }
    return 0;
}

int32_t fs_bla_num_levels(const fs_renderer *r) { return r->bla_n_levels; }
int32_t fs_bla_lm2(const fs_renderer *r) { return r->bla_lm2; }
uint64_t fs_bla_level_size(const fs_renderer *r, int32_t level)
{
    return level >= 0 && (size_t)level < r->bla_level_sizes.size() ? r->bla_level_sizes[(size_t)level] : 0;
}
uint32_t fs_read_ndz_bounds(fs_renderer *r, float *bounds_out, float *entries_out, uint64_t max_entries, uint64_t *n_out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->zq || !r->znz || !r->zq_n)
        return FS_ERR_6;
    const uint64_t n = r->zq_n < max_entries ? r->zq_n : max_entries;
    if (bounds_out && n)
        FS_TRY(hipMemcpyAsync(bounds_out, r->znz, n * sizeof(float2), hipMemcpyDeviceToHost, r->compute));
    if (entries_out && n)
        FS_TRY(hipMemcpyAsync(entries_out, r->zq + r->zq_n, n * sizeof(float4), hipMemcpyDeviceToHost, r->compute));
    if (n_out)
        *n_out = r->zq_n;
    return (uint32_t)hipStreamSynchronize(r->compute);
}

uint32_t fs_read_quiet_orbit(fs_renderer *r, int part, void *out, uint64_t max_bytes, uint64_t *bytes)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->compute)
        return FS_ERR_6;
    const bool expanded = r->orbit_ok && !r->orbit_seq;
    const bool hdr32 = expanded && r->orbit_type == FS_T_HDR32 && r->zref && r->zq && r->zq_n;
    const uint64_t m = r->zq_n, slack = kQuietSlack;
    const void *src = nullptr;
    uint64_t n = 0;
    bool made = hdr32;
    switch (part) {
        case FS_QUIET_PART_PREPARED: src = r->zref, n = m * sizeof(float4); break;
        case FS_QUIET_PART_FIRST: src = r->zq, n = m * sizeof(float4); break;
        case FS_QUIET_PART_SECOND: src = r->zq + m, n = m * sizeof(float4); break;
        case FS_QUIET_PART_ZS2: src = r->zs2, n = (m + slack) * sizeof(float2); break;
        case FS_QUIET_PART_ZQB: src = r->zqb, n = (m + slack) * sizeof(float4); break;
        case FS_QUIET_PART_ZNZ: src = r->znz, n = (m + slack) * sizeof(float2); break;
        case FS_QUIET_PART_PREPARED64:
            made = expanded && r->orbit_type == FS_T_HDR64 && r->zref64;
            src = r->zref64, n = (r->orbit_uncompressed + 2) * sizeof(FsZ64);
            break;
        case FS_QUIET_PART_SCALED_F32:
            made = r->scaled_f && r->scaled_count;
            src = r->scaled_f, n = r->scaled_count * sizeof(fs_orbit_f32_bad);
            break;
        default: return FS_ERR_7;
    }
    if (!made)
        return FS_ERR_6;
    if (bytes)
        *bytes = n;
    const uint64_t c = n < max_bytes ? n : max_bytes;
    if (out && c)
        FS_TRY(hipMemcpyAsync(out, src, (size_t)c, hipMemcpyDeviceToHost, r->compute));
    return (uint32_t)hipStreamSynchronize(r->compute);
}

uint32_t fs_read_bla_level(fs_renderer *r, int32_t level, void *out, uint64_t max_records)
{
    if (uint32_t e = use_device(r))
        return e;
    if (level < 0 || (size_t)level >= r->bla_level_mem.size())
        return FS_ERR_7;
    const size_t rec_bytes = r->bla_type == FS_T_HDR32 ? sizeof(fs_bla_hdr32)
                                                       : (r->bla_type == FS_T_HDR64 ? sizeof(fs_bla_hdr64) : sizeof(fs_bla_f64));
    const uint64_t n = r->bla_level_sizes[(size_t)level] < max_records ? r->bla_level_sizes[(size_t)level] : max_records;
    if (n && r->bla_level_mem[(size_t)level])
        FS_TRY(hipMemcpyAsync(out, r->bla_level_mem[(size_t)level], n * rec_bytes, hipMemcpyDefault, r->compute));
    return (uint32_t)hipStreamSynchronize(r->compute);
}

// The device-native forms of the installed HDRFloat<float> table, made first when they are stale (as fs_render_bla does).
static uint32_t bla_native_current(fs_renderer *r)
{
    if (r->bla_native_stale && r->bla_n_levels > 2 && r->bla_levels_dev != nullptr && r->bla_type == FS_T_HDR32)
        return bla_make_native(r, r->bla_n_levels);
    return 0;
}

uint32_t fs_read_bla_native(fs_renderer *r, int part, void *out, uint64_t max_bytes, uint64_t *bytes)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->compute || r->bla_type != FS_T_HDR32)
        return FS_ERR_6;
    if (uint32_t e = bla_native_current(r))
        return e;
    const bool native = r->bla_native_ok && !r->bla_native_stale && r->bla_n_levels > 2, heap = native && r->bla_heap_ok;
    const uint64_t total = native ? r->bla_native_total : 0, hn = heap ? r->bla_heap_positions : 0;
    const uint64_t n_q = (uint64_t)(r->orbit_uncompressed / 4u) + 2u; // (bla_make_native's n_kmax)
    uint32_t geom[16 + 2 * kBlaMaxLevels];
    memset(geom, 0, sizeof(geom));
    const void *src = nullptr;
    uint64_t n = 0;
    const char *nat = r->bla_native.as<const char>() + 256, *hp = r->bla_heap.as<const char>();
    switch (part) {
        case FS_BLA_PART_GEOMETRY: {
            geom[0] = native, geom[1] = heap, geom[2] = (uint32_t)r->bla_n_levels, geom[3] = (uint32_t)r->bla_lm2;
            geom[4] = (uint32_t)total, geom[6] = (uint32_t)hn, geom[7] = native ? (uint32_t)n_q : 0u;
            geom[8] = (uint32_t)r->orbit_uncompressed;
            for (uint64_t h = hn; h != 0; h >>= 1) // positions = 2^(H - 1)
                geom[5]++;
            for (int32_t l = 2; native && l < r->bla_n_levels && l < kBlaMaxLevels; l++) {
                geom[16 + l] = r->bla_level_off[l];
                geom[16 + kBlaMaxLevels + l] = (uint32_t)r->bla_level_sizes[(size_t)l];
            }
            if (bytes)
                *bytes = sizeof(geom);
            if (out)
                memcpy(out, geom, max_bytes < sizeof(geom) ? (size_t)max_bytes : sizeof(geom));
            return 0;
        }
        case FS_BLA_PART_RECORDS: src = nat, n = total * sizeof(FsBlaRec); break;
        case FS_BLA_PART_LADDER: src = nat + total * sizeof(FsBlaRec), n = total * 2 * sizeof(int4); break;
        case FS_BLA_PART_PRETEST:
            src = nat + total * (sizeof(FsBlaRec) + 2 * sizeof(int4)), n = native ? n_q * sizeof(long long) : 0;
            break;
        case FS_BLA_PART_HEAP_RECORDS: src = hp, n = hn * sizeof(FsBlaRec); break;
        case FS_BLA_PART_HEAP_LADDER: src = hp + hn * sizeof(FsBlaRec), n = hn * 2 * sizeof(int4); break;
        case FS_BLA_PART_Q: src = hp + hn * (sizeof(FsBlaRec) + 2 * sizeof(int4)), n = heap ? n_q * 3 * sizeof(int4) : 0; break;
        case FS_BLA_PART_ZB:
            src = hp + hn * (sizeof(FsBlaRec) + 2 * sizeof(int4)) + n_q * 3 * sizeof(int4);
            n = heap ? (r->orbit_uncompressed + 2u) * sizeof(float4) : 0;
            break;
        default: return FS_ERR_7;
    }
    if (part >= FS_BLA_PART_HEAP_RECORDS ? !heap : !native)
        return FS_ERR_6;
    if (bytes)
        *bytes = n;
    const uint64_t c = n < max_bytes ? n : max_bytes;
    if (out && c)
        FS_TRY(hipMemcpyAsync(out, src, (size_t)c, hipMemcpyDeviceToHost, r->compute));
    return (uint32_t)hipStreamSynchronize(r->compute);
}

uint32_t fs_bla_lookup_probe(fs_renderer *r, int which, const uint32_t *m, const void *z2, uint32_t n, uint32_t *level_ix_out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (which < 0 || which > 2 || !m || !z2 || !level_ix_out || n > 0x7FFFFF00u)
        return hipErrorInvalidValue;
    if (!r->compute || r->bla_n_levels <= 2 || r->bla_levels_dev == nullptr || r->bla_type != (which == 1 ? FS_T_HDR64 : FS_T_HDR32) ||
        r->bla_level_sizes.size() < 3 || r->bla_level_sizes[2] == 0)
        return FS_ERR_6;
    // every index a walk forms stays inside its level when (m - 1) >> 2 names an element of level 2
    for (uint32_t i = 0; i < n; i++)
        if (m[i] != 0u && (uint64_t)(m[i] - 1u) >= 4u * r->bla_level_sizes[2])
            return FS_ERR_7;
    if (which == 2) {
        if (uint32_t e = bla_native_current(r))
            return e;
        if (!r->bla_native_ok || r->bla_native_stale)
            return FS_ERR_6;
    }
    if (n == 0)
        return 0;
    const size_t zb = which == 1 ? sizeof(fs_real_hdr64) : sizeof(fs_real_hdr32);
    const uint32_t np = (n + 255u) & ~255u; // full waves: the native lookup votes across the wave
    char *dev = nullptr;
    const size_t m_bytes = (size_t)np * sizeof(uint32_t), z_bytes = (size_t)np * zb, o_bytes = (size_t)np * 2 * sizeof(uint32_t);
    FS_TRY(r_alloc(r, &dev, m_bytes + z_bytes + o_bytes, kFrame));
    uint32_t *dm = (uint32_t *)(dev + z_bytes + o_bytes), *dout = (uint32_t *)(dev + z_bytes); // (z2 first: 8-byte aligned)
    hipError_t err = hipMemsetAsync(dev, 0, m_bytes + z_bytes + o_bytes, r->compute); // the padding asks m = 0
    if (err == hipSuccess)
        err = hipMemcpyAsync(dm, m, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, r->compute);
    if (err == hipSuccess)
        err = hipMemcpyAsync(dev, z2, (size_t)n * zb, hipMemcpyHostToDevice, r->compute);
    if (err == hipSuccess) {
        const char *nat = r->bla_native.as<const char>() + 256;
        const int4 *nlad = (const int4 *)(nat + (size_t)r->bla_native_total * sizeof(FsBlaRec));
        fsk_bla_lookup_probe(which, (const void *const *)r->bla_levels_dev, nlad,
                             (const long long *)(nlad + 2 * (size_t)r->bla_native_total), which == 2 ? r->bla_level_off : nullptr,
                             r->bla_level_sizes.data(), r->bla_n_levels, r->bla_lm2, dm, dev, np, dout, r->compute);
        err = hipGetLastError();
    }
    if (err == hipSuccess)
        err = hipMemcpyAsync(level_ix_out, dout, (size_t)n * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, r->compute);
    if (err == hipSuccess)
        err = hipStreamSynchronize(r->compute);
    else
        (void)hipStreamSynchronize(r->compute);
    (void)r_free(r, dev);
    return (uint32_t)err;
}

uint32_t fs_set_compressed_orbit_mode(fs_renderer *r, int mode)
{
    if (mode != 0 && mode != 1)
        return hipErrorInvalidValue;
    r->compressed_mode = mode;
    return 0;
}

uint64_t fs_orbit_device_bytes(const fs_renderer *r)
{
    if (!r->orbit_ok)
        return 0;
    const uint64_t n = r->orbit_uncompressed;
    if (r->orbit_seq) {
        switch (r->orbit_type) {
            case FS_T_HDR32: return r->orbit_size * sizeof(fs_orbit_hdr32_rc);
            case FS_T_HDR64: return r->orbit_size * sizeof(fs_orbit_hdr64_rc);
            case FS_T_F32: return r->orbit_size * sizeof(fs_orbit_f32_rc);
            case FS_T_F64: return r->orbit_size * sizeof(fs_orbit_f64_rc);
            case FS_T_2X32: return r->orbit_size * sizeof(fs_orbit_p2x32_rc);
            default: return r->orbit_size * sizeof(fs_orbit_2x32_rc);
        }
    }
    switch (r->orbit_type) {
        case FS_T_HDR32: // prepared entries + the two companion arrays of the tuned loops
            return (n + 2) * sizeof(float4) + quiet_orbit_units(n) * sizeof(float4);
        case FS_T_HDR64:
            return (n + 2) * sizeof(FsZ64);
        case FS_T_F64:
            return n * sizeof(fs_orbit_f64);
        case FS_T_HDR2X32:
            return n * sizeof(fs_orbit_2x32);
        case FS_T_F32:
            return (n + 1) * sizeof(fs_orbit_f32);
        case FS_T_2X32:
            return (n + 1) * sizeof(fs_orbit_p2x32);
        default:
            return 0;
    }
}

} // extern "C"
