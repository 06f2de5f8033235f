// renderer_current.cpp -- RenderCurrent: the frame as it stands, coloured, reduced and copied to the host.
#include "renderer_state.hpp"

using namespace fsr;

extern "C" {

uint32_t fs_clear(fs_renderer *r)
{
    if (uint32_t e = use_device(r))
        return e;
    exact_drop_kept(r);
    if (!r->memory_initialized())
        return 0;
    const size_t elems = (size_t)r->w_block * 16u * r->local_rows_padded;
    FS_TRY(hipMemsetAsync(r->iters(), 0, elems * r->iter_bytes, r->compute));
    if (r->colors)
        FS_TRY(hipMemsetAsync(r->colors, 0, r->n_color_cu * sizeof(fs_color16), r->compute));
    return 0;
}

uint32_t fs_render_current(fs_renderer *r, uint64_t n_iterations, void *iter_buffer, fs_color16 *color_buffer,
                           fs_reduction *reduction, int progressive)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->memory_initialized())
        return 0; // GPU_Render.cu:564-566
    hipStream_t s = progressive ? r->display : r->compute;
    const uint32_t rw = r->w_block * 16u;
    const bool whole_frame = r->local_rows == r->height;
    if (color_buffer && r->pal && whole_frame) {
        fsk_antialias(r->iters(), r->iter_bytes == 8, rw, r->colors, r->pal, r->pal_iters, r->pal_aux_depth, r->aa,
                      r->color_w, r->color_h, n_iterations, s);
        FS_TRY(hipGetLastError());
    }
    if (reduction) {
        r->reduce_seed = fs_reduction{r->iter_bytes == 8 ? ~0ull : 0xFFFFFFFFull, 0, 0}; // ReductionKernels.cuh:99-104
        FS_TRY(hipMemcpyAsync(r->reduction, &r->reduce_seed, sizeof(fs_reduction), hipMemcpyHostToDevice, s));
        fsk_reduce(r->iters(), r->iter_bytes == 8, rw, r->width, r->local_rows, r->reduction, s);
        FS_TRY(hipGetLastError());
    }
    // ExtractItersAndColors, GPU_Render.cu:1759-1805: padding included.
    if (iter_buffer)
        FS_TRY(hipMemcpyAsync(iter_buffer, r->iters(), (size_t)rw * r->local_rows_padded * r->iter_bytes,
                              hipMemcpyDefault, s));
    if (color_buffer && whole_frame)
        FS_TRY(hipMemcpyAsync(color_buffer, r->colors, r->n_color_cu * sizeof(fs_color16), hipMemcpyDefault, s));
    if (reduction)
        FS_TRY(hipMemcpyAsync(reduction, r->reduction, sizeof(fs_reduction), hipMemcpyDefault, s));
    return 0;
}

uint32_t fs_time_render_current(fs_renderer *r, uint64_t n_iterations, uint32_t repeats, float ms_out[2])
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->memory_initialized() || !r->pal || r->local_rows != r->height || !repeats)
        return FS_ERR_6;
    const uint32_t rw = r->w_block * 16u;
    hipEvent_t a, b;
    FS_TRY(hipEventCreate(&a));
    FS_TRY(hipEventCreate(&b));
    // the kernels only (the 24-byte seed copy of fs_render_current is not part of what is measured; min / max are
    // idempotent and the accumulated sum of the repeats is discarded)
    r->reduce_seed = fs_reduction{r->iter_bytes == 8 ? ~0ull : 0xFFFFFFFFull, 0, 0};
    FS_TRY(hipMemcpyAsync(r->reduction, &r->reduce_seed, sizeof(fs_reduction), hipMemcpyHostToDevice, r->compute));
    for (int which = 0; which < 2; which++) {
        FS_TRY(hipEventRecord(a, r->compute));
        for (uint32_t i = 0; i < repeats; i++) {
            if (which == 0)
                fsk_antialias(r->iters(), r->iter_bytes == 8, rw, r->colors, r->pal, r->pal_iters, r->pal_aux_depth, r->aa,
                              r->color_w, r->color_h, n_iterations, r->compute);
            else
                fsk_reduce(r->iters(), r->iter_bytes == 8, rw, r->width, r->local_rows, r->reduction, r->compute);
        }
        FS_TRY(hipEventRecord(b, r->compute));
        FS_TRY(hipEventSynchronize(b));
        FS_TRY(hipGetLastError());
        float ms = 0;
        FS_TRY(hipEventElapsedTime(&ms, a, b));
        ms_out[which] = ms / (float)repeats;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return 0;
}

// RunAntialiasing (GPU_Render.cu:1695-1757) over a whole frame that lies somewhere else on this renderer's device (the frame
// an fs_group has put back in row order), with this renderer's palette and geometry, on the caller's stream.
uint32_t fs_colorize_frame(fs_renderer *r, const void *device_iters, uint64_t n_iterations, fs_color16 *device_colors,
                           fs_color16 *color_buffer, void *stream)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->memory_initialized() || !device_iters)
        return 0;
    if (!r->pal)
        return 0; // no palette was ever uploaded: RenderCurrent leaves the colour buffer alone
    hipStream_t s = (hipStream_t)stream;
    fs_color16 *dst = device_colors ? device_colors : r->colors;
    fsk_antialias(device_iters, r->iter_bytes == 8, r->w_block * 16u, dst, r->pal, r->pal_iters, r->pal_aux_depth, r->aa,
                  r->color_w, r->color_h, n_iterations, s);
    FS_TRY(hipGetLastError());
    if (color_buffer)
        FS_TRY(hipMemcpyAsync(color_buffer, dst, r->n_color_cu * sizeof(fs_color16), hipMemcpyDefault, s));
    return 0;
}
uint64_t fs_color_buffer_elements(const fs_renderer *r) { return r->n_color_cu; }

uint32_t fs_read_color_buffer(fs_renderer *r, fs_color16 *out)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->memory_initialized() || !r->colors || !out)
        return FS_ERR_6;
    FS_TRY(hipMemcpyAsync(out, r->colors, r->n_color_cu * sizeof(fs_color16), hipMemcpyDeviceToHost, r->compute));
    FS_TRY(hipStreamSynchronize(r->compute));
    return 0;
}

// The renderer's bands -> their rows of a WHOLE-FRAME host buffer, over THIS device's own PCIe link (round 6; the sharded
// read-back of the row-tiled frame: GPURenderer::ExtractItersAndColors, GPU_Render.cu:1760-1805, copies N_cu counts per frame
// through one device).  The local buffer holds the owned bands back to back and band k belongs at frame row
// band_first + k * band_stride: ONE two-dimensional copy whose "row" is a whole band (band_rows x pitch bytes) and whose
// destination pitch is the band stride, so the rows land in frame order and nothing has to restore it; a last, shorter band
// goes by itself.
uint32_t fs_copy_bands_to_host(fs_renderer *r, const void *device_iters, void *host_frame, void *stream)
{
    if (uint32_t e = use_device(r))
        return e;
    if (!r->memory_initialized() || !host_frame)
        return host_frame ? 0u : (uint32_t)hipErrorInvalidValue;
    if (r->local_rows == 0)
        return 0;
    const char *src = (const char *)(device_iters ? device_iters : r->iters());
    hipStream_t s = stream ? (hipStream_t)stream : r->compute;
    const size_t pitch = (size_t)r->w_block * 16u * r->iter_bytes;
    const uint64_t H = r->height, first = r->band_first, rows = r->band_rows, stride = r->band_stride;
    if (first == 0 && rows >= H) // no banding: the whole padded buffer, as fs_render_current copies it
        return (uint32_t)hipMemcpyAsync(host_frame, src, (size_t)r->local_rows_padded * pitch, hipMemcpyDeviceToHost, s);
    uint64_t full = 0; // bands that lie wholly inside the frame
    if (first + rows <= H)
        full = (H - rows - first) / stride + 1u;
    char *dst = (char *)host_frame + first * pitch;
    if (full == 1u || (full > 1u && stride == rows)) {
        FS_TRY(hipMemcpyAsync(dst, src, full * rows * pitch, hipMemcpyDeviceToHost, s));
    } else if (full > 1u) {
        FS_TRY(hipMemcpy2DAsync(dst, stride * pitch, src, rows * pitch, rows * pitch, full, hipMemcpyDeviceToHost, s));
    }
    const uint64_t tail_start = first + full * stride;
    if (tail_start < H) { // the last band is cut by the frame's edge
        const uint64_t tail_rows = (tail_start + rows < H ? tail_start + rows : H) - tail_start;
        FS_TRY(hipMemcpyAsync((char *)host_frame + tail_start * pitch, src + full * rows * pitch, tail_rows * pitch,
                              hipMemcpyDeviceToHost, s));
    }
    return 0;
}

} // extern "C"
