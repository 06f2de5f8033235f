// arith_device.hip -- the gfx950 device pass of the arithmetic headers on a file of cases (see arith_ops.hpp): a stand-alone
// program, built by tests/test_gpu_arith_edges.py with exactly the product's render flags.  One launch per op family, one case per
// lane; every lane reads its own 17 words and writes its own 8.
//   arith_device cases.bin out.bin
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "arith_ops.hpp"

using namespace arith;

#define CHECK(call)                                                                                                       \
    do {                                                                                                                  \
        const hipError_t e_ = (call);                                                                                     \
        if (e_ != hipSuccess) {                                                                                           \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));                          \
            return 1;                                                                                                     \
        }                                                                                                                 \
    } while (0)

// cases [first, first + count) of `in` (17 words each) into the same rows of `out` (8 words each); a case whose id is not in the
// family's table leaves its row as it is (zeros)
#define ARITH_KERNEL(FAM, lo, hi)                                                                                         \
    __global__ void __launch_bounds__(64) k_##FAM(const uint32_t *in, uint32_t *out, uint32_t first, uint32_t count)      \
    {                                                                                                                     \
        const uint32_t i = blockIdx.x * 64u + threadIdx.x;                                                                \
        if (i >= count)                                                                                                   \
            return;                                                                                                       \
        const uint32_t *p = in + (size_t)(first + i) * kCaseWords;                                                        \
        uint32_t *o = out + (size_t)(first + i) * kOutWords;                                                              \
        switch (*p++) {                                                                                                   \
            ARITH_OPS_##FAM(ARITH_CASE)                                                                                   \
        default:                                                                                                          \
            break;                                                                                                        \
        }                                                                                                                 \
    }
ARITH_FAMILIES(ARITH_KERNEL)

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: arith_device cases.bin out.bin\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 3;
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n == 0 || n > (1u << 22))
        return 3;
    std::vector<uint32_t> in((size_t)n * kCaseWords), res((size_t)n * kOutWords, 0u);
    if (fread(in.data(), 4, in.size(), f) != in.size())
        return 3;
    fclose(f);
    // the cases are sorted by id, so a family is one contiguous run of rows
    for (uint32_t i = 1; i < n; ++i)
        if (in[(size_t)i * kCaseWords] < in[(size_t)(i - 1) * kCaseWords])
            return 3;

    uint32_t *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * 4));
    CHECK(hipMalloc(&d_out, res.size() * 4));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, res.size() * 4));
#define ARITH_LAUNCH(FAM, lo, hi)                                                                                         \
    {                                                                                                                     \
        uint32_t first = 0, last = 0;                                                                                     \
        while (first < n && in[(size_t)first * kCaseWords] < (uint32_t)(lo))                                              \
            ++first;                                                                                                      \
        last = first;                                                                                                     \
        while (last < n && in[(size_t)last * kCaseWords] <= (uint32_t)(hi))                                               \
            ++last;                                                                                                       \
        if (last > first) {                                                                                               \
            k_##FAM<<<dim3((last - first + 63u) / 64u), dim3(64), 0, 0>>>(d_in, d_out, first, last - first);             \
            CHECK(hipGetLastError());                                                                                     \
            CHECK(hipDeviceSynchronize());                                                                                \
        }                                                                                                                 \
    }
    ARITH_FAMILIES(ARITH_LAUNCH)
    CHECK(hipMemcpy(res.data(), d_out, res.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(res.data(), 4, res.size(), f) != res.size() || fclose(f) != 0)
        return 4;
    return 0;
}
