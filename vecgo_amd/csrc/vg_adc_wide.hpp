// vg_adc_wide.hpp — the PQ table sums of a batch of tiles against a table that one LDS image does not hold (fp32 table of m KiB:
// m > 96 next to the scans' buffers; d = 1536 at 8 dimensions per sub-quantizer is m = 192).
//
// The table is walked in CHUNKS of up to kWideChunkGroups full groups (96 KiB): a workgroup takes a batch of kWideTiles tiles per
// wave, keeps their 16 slot accumulators in registers (kWideTiles * 16 VGPRs), and for each chunk stages that chunk's table rows
// into LDS between two barriers and adds the chunk's groups for every wanted tile of the batch.  Every row still adds its groups
// in ascending order into the same 16 accumulators, then the _mm512_reduce_add_ps tree, then the m % 16 tail in order: the sum is
// pqAdcLookupAvx512's (vg_adc_row.hpp), bit for bit what adc_row_score_lds gives against a whole image.  The table is re-staged
// once per batch (m KiB from L2 against WAVES * kWideTiles * 64 * m bytes of codes: a quarter of the code traffic at 4 tiles per
// wave and 8 waves).
//
// One copy of the walk for pq_adc_scan_wide_kernel, pq_adc_probe_wide_kernel (k_adc.hip) and pthr_scan_wide_kernel
// (k_probed_threshold.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "vg_adc_row.hpp"
#include "vg_device.hpp"

namespace vg {

constexpr int kWideTiles = 4;
constexpr int kWideChunkGroups = 6;
constexpr int kWideChunkWords = (kWideChunkGroups / 2) * 8192;
constexpr int kWideLdsWords = kWideChunkWords + 15 * 256;  // one chunk [pair][c][32], then the m % 16 natural rows [j][c]

// Tile tb of the calling wave is b0 + tb * WAVES + wave.  want[tb] (wave-uniform): the tile's sums are asked for — a tile that is
// not wanted reads no code bytes and leaves total[tb] alone; a batch no wave wants anything of stages nothing.  image: the query's
// table image (lut_image_words(m) words, 16-byte aligned); lut: kWideLdsWords words of LDS, the walker's from its first barrier to
// its return.  EVERY thread of the workgroup (WAVES * 64) calls with the same b0, m and image: the walk has workgroup barriers.
template <int WAVES>
__device__ __forceinline__ void adc_wide_walk(const uint4 *__restrict__ tiles, int groups, int m, const float *__restrict__ image,
                                              float *lut, int64_t b0, const bool (&want)[kWideTiles], int tid,
                                              float (&total)[kWideTiles])
{
    constexpr int kThreads = WAVES * 64;
    const int lane = tid & 63, wave = tid >> 6, rot = lane & 15;
    const int gfull = m >> 4, tail = m & 15;
    const int nchunks = gfull ? (gfull + kWideChunkGroups - 1) / kWideChunkGroups : 1;
    const int tail_word = ((gfull + 1) >> 1) * 8192;
    float *lut_tail = lut + kWideChunkWords;
    bool any = false;
#pragma unroll
    for (int tb = 0; tb < kWideTiles; tb++) any = any || want[tb];
    // (also the barrier behind the previous batch's tail reads)
    if (!__syncthreads_or(any)) return;
    float acc[kWideTiles][16];
#pragma unroll
    for (int tb = 0; tb < kWideTiles; tb++)
#pragma unroll
        for (int l = 0; l < 16; l++) acc[tb][l] = 0.0f;
    for (int c = 0; c < nchunks; c++) {
        const int g0 = c * kWideChunkGroups;
        const int gc = gfull - g0 < kWideChunkGroups ? gfull - g0 : kWideChunkGroups;
        if (c) __syncthreads();  // the previous chunk's lookups are done
        {
            const int words = ((gc + 1) >> 1) * 8192;
            const float4 *src = reinterpret_cast<const float4 *>(image + (g0 >> 1) * 8192);
            float4 *dst = reinterpret_cast<float4 *>(lut);
            for (int i = tid; i < words / 4; i += kThreads) dst[i] = src[i];
            if (c == nchunks - 1 && tail) {
                const float4 *ts = reinterpret_cast<const float4 *>(image + tail_word);
                float4 *td = reinterpret_cast<float4 *>(lut_tail);
                for (int i = tid; i < tail * 64; i += kThreads) td[i] = ts[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int tb = 0; tb < kWideTiles; tb++) {
            if (want[tb]) {
                const int64_t tile = b0 + static_cast<int64_t>(tb) * WAVES + wave;
                const uint4 *tp = tiles + (tile * groups) * 64 + lane;
                for (int g = 0; g < gc; g++) {
                    const uint4 cw = tp[(g0 + g) * 64];
#pragma unroll
                    for (int sl = 0; sl < 16; sl++)
                        acc[tb][sl] = acc[tb][sl] + lut[((g >> 1) * 256 + code_byte(cw, sl)) * 32 + (g & 1) * 16 + ((sl + rot) & 15)];
                }
            }
        }
    }
#pragma unroll
    for (int tb = 0; tb < kWideTiles; tb++) {
        if (want[tb]) {
            const int64_t tile = b0 + static_cast<int64_t>(tb) * WAVES + wave;
            float t = reduce16_regs(acc[tb]);
            if (tail) {
                const uint4 cw = tiles[(tile * groups + gfull) * 64 + lane];
                for (int l = 0; l < tail; l++) t = t + lut_tail[l * 256 + code_byte(cw, l)];
            }
            total[tb] = t;
        }
    }
}

}  // namespace vg
