// vg_adc_row.hpp — one row's PQ table sum from the re-tiled codes and a query's LUT image in LDS (k_adc.hip's layouts):
// pqAdcLookupAvx512 order (internal/simd/src/floats_avx512.c:135-167) — 16 lane accumulators over the full 16-wide groups,
// the _mm512_reduce_add_ps tree, the m % 16 tail added in order.  The plain gather loop of the partition-probed scan
// (pq_adc_probe_kernel) and of the threshold scan (k_probed_threshold.hip); the exhaustive scan hand-pipelines the same reads.
#pragma once

#include <hip/hip_runtime.h>

#include "vg_device.hpp"

namespace vg {

__device__ __forceinline__ uint32_t code_byte(const uint4 &c, int l)
{
    uint32_t w = (l < 4) ? c.x : (l < 8) ? c.y : (l < 12) ? c.z : c.w;
    return (w >> (8 * (l & 3))) & 0xFFu;
}

// words of the per-query LUT image (pair-interleaved full groups + natural tail rows)
__host__ __device__ inline int lut_image_words(int m) { return (((m >> 4) + 1) >> 1) * 8192 + (m & 15) * 256; }

// tp: the lane's 16-byte piece of group 0 of its row's tile (tiles + (tile * groups) * 64 + lane); rot = lane & 15
__device__ __forceinline__ float adc_row_score_lds(const float *lut, const uint4 *__restrict__ tp, int m, int rot)
{
    const int gfull = m >> 4, tail = m & 15;
    float acc[16];
#pragma unroll
    for (int l = 0; l < 16; l++) acc[l] = 0.0f;
    for (int g = 0; g < gfull; g++) {
        const uint4 c = tp[g * 64];
#pragma unroll
        for (int sl = 0; sl < 16; sl++)
            acc[sl] = acc[sl] + lut[((g >> 1) * 256 + code_byte(c, sl)) * 32 + (g & 1) * 16 + ((sl + rot) & 15)];
    }
    float total = reduce16_regs(acc);
    if (tail) {
        const int lut_tail_word = ((gfull + 1) >> 1) * 8192;
        const uint4 c = tp[gfull * 64];
        for (int l = 0; l < tail; l++) total = total + lut[lut_tail_word + l * 256 + code_byte(c, l)];
    }
    return total;
}

}  // namespace vg
