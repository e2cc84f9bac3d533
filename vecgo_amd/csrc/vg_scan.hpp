// vg_scan.hpp — the 64-bit workgroup prefix sum and the segment prefix kernel that the mask compaction (k_prefilter.hip) and
// the BM25 index update (k_bm25_update.hip) rank with.  (vg_permute.hpp holds the 32-bit form of the reorder passes.)
#pragma once

#include "vg_internal.hpp"

namespace vg {

constexpr int kScanThreads = 256;

// the workgroup's inclusive prefix of x at this thread and the workgroup's total (all kScanThreads threads call; wsum: one
// slot per wave)
__device__ __forceinline__ long long block_scan(long long x, long long *wsum, long long &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
    }
    __syncthreads();  // the previous use of wsum has been read
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long before = 0;
    total = 0;
    for (int w = 0; w < kScanThreads / 64; w++) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    return before + inc;
}

// segment blockIdx.x of v (n values each) <- its exclusive prefix sums, in place; the segment's total to tot64 / tot32
template <typename T>
__global__ __launch_bounds__(kScanThreads) void prefix_kernel(T *__restrict__ v, int64_t n, int64_t *__restrict__ tot64, int *__restrict__ tot32)
{
    __shared__ long long wsum[kScanThreads / 64];
    T *p = v + static_cast<int64_t>(blockIdx.x) * n;
    long long carry = 0;
    for (int64_t i0 = 0; i0 < n; i0 += kScanThreads) {
        const int64_t i = i0 + threadIdx.x;
        const long long x = i < n ? static_cast<long long>(p[i]) : 0;
        long long total;
        const long long inc = block_scan(x, wsum, total);
        if (i < n) p[i] = static_cast<T>(carry + inc - x);
        carry += total;
    }
    if (threadIdx.x == 0) {
        if (tot64) tot64[blockIdx.x] = carry;
        if (tot32) tot32[blockIdx.x] = static_cast<int>(carry);
    }
}

}  // namespace vg
