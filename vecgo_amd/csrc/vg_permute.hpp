// vg_permute.hpp — what the two writers that reorder a resident index share (k_vamana_reorder.hip: the DiskANN writer's BFS
// order; k_flat_build.hip: the flat writer's partition order): the workgroup prefix sum their placement passes rank with, and
// the gather that moves a per-row array of any row size into the new order.
#pragma once

#include <algorithm>

#include "vg_internal.hpp"

namespace vg {

constexpr int kRbThreads = 256;

// exclusive prefix of `cnt` over the workgroup (kRbThreads threads) in thread order; *total = the sum.  Ends with a barrier.
__device__ __forceinline__ uint32_t rb_block_scan(uint32_t cnt, uint32_t *wsum, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = cnt;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < kRbThreads / 64; w++) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    __syncthreads();
    *total = all;
    return before + incl - cnt;
}

// dst row q = src row perm[q], rows of `words` W-byte words
template <typename W>
__global__ __launch_bounds__(256) void rb_gather_kernel(const W *__restrict__ src, W *__restrict__ dst, int64_t n, int64_t words,
                                                        const uint32_t *__restrict__ perm)
{
    const int64_t total = n * words;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t q = e / words, k = e - q * words;
        dst[e] = src[static_cast<int64_t>(perm[q]) * words + k];
    }
}

static unsigned rb_grid(int64_t total)
{
    return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 8192)));
}

// the widest access that divides a row (rows start at a hipMalloc'd base: a word of that size is aligned in every row)
static int64_t rb_word_bytes(int64_t row_bytes)
{
    return row_bytes % 16 == 0 ? 16 : row_bytes % 8 == 0 ? 8 : row_bytes % 4 == 0 ? 4 : row_bytes % 2 == 0 ? 2 : 1;
}

// array <- array gathered by perm, through scratch; row_bytes of any size, the widest access that divides it
static int32_t rb_permute_rows(void *array, int64_t n, int64_t row_bytes, const uint32_t *perm, void *scratch, hipStream_t st)
{
    if (!array || n == 0 || row_bytes == 0) return VG_OK;
    const int64_t w = rb_word_bytes(row_bytes);
    const int64_t words = row_bytes / w;
    const unsigned grid = rb_grid(n * words);
#define VG_RB_GATHER(T) \
    VG_LAUNCH(rb_gather_kernel<T>, dim3(grid), dim3(256), 0, st, static_cast<const T *>(array), static_cast<T *>(scratch), n, words, perm)
    switch (w) {
        case 16: VG_RB_GATHER(uint4); break;
        case 8: VG_RB_GATHER(uint2); break;
        case 4: VG_RB_GATHER(uint32_t); break;
        case 2: VG_RB_GATHER(uint16_t); break;
        default: VG_RB_GATHER(uint8_t); break;
    }
#undef VG_RB_GATHER
    VG_HIP(hipMemcpyAsync(array, scratch, static_cast<size_t>(n * row_bytes), hipMemcpyDeviceToDevice, st));
    return VG_OK;
}

}  // namespace vg
