// vg_sq8_row.hpp — the arithmetic of one SQ8 row, DEVICE ONLY: what the quantizer's batch kernels (k_sq8.hip) and the index
// scan, its verify pair and its NaN replay (k_sq8_scan.hip) both score a row with.  The numerics contract is k_sq8.hip's.
#pragma once

#include "vg_device.hpp"

namespace vg {

// ---- the row kernel --------------------------------------------------------------------------------
// 16 bytes = one 16-element block of one row: lane accumulators l = 0..15 get one FMA each.
// qv / mn / iv point at the block's 16 floats and are wave-uniform.
__device__ __forceinline__ void sq8_block16(float (&acc)[16], const uint4 c, const float *__restrict__ qv,
                                            const float *__restrict__ mn, const float *__restrict__ iv)
{
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int l = 0; l < 16; l++) {
        const float cf = static_cast<float>((w[l >> 2] >> (8 * (l & 3))) & 0xFFu);
        const float rec = __builtin_fmaf(cf, iv[l], mn[l]);
        const float diff = qv[l] - rec;
        acc[l] = __builtin_fmaf(diff, diff, acc[l]);
    }
}

// the tail of a row (dim % 16 elements, bytes in the low lanes of the last group)
__device__ __forceinline__ float sq8_tail(float total, const uint4 c, int cnt, const float *__restrict__ qv,
                                          const float *__restrict__ mn, const float *__restrict__ iv)
{
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
    for (int l = 0; l < cnt; l++) {
        const float cf = static_cast<float>((w[l >> 2] >> (8 * (l & 3))) & 0xFFu);
        const float rec = __builtin_fmaf(cf, iv[l], mn[l]);
        const float diff = qv[l] - rec;
        total = __builtin_fmaf(diff, diff, total);
    }
    return total;
}

// ScalarQuantizer.DotProduct (quantizer.go:109-119) over `cnt` (<= 16) elements of one row: a plain Go
// loop — val = mins[i] + float32(code[i])*invScales[i], dot += q[i]*val, four separately rounded
// operations (no FMA on amd64), one running sum in element order.
__device__ __forceinline__ float sq8_dot16(float total, const uint4 c, int cnt, const float *__restrict__ qv,
                                           const float *__restrict__ mn, const float *__restrict__ iv)
{
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int l = 0; l < 16; l++) {
        if (l < cnt) {
            const float cf = static_cast<float>((w[l >> 2] >> (8 * (l & 3))) & 0xFFu);
            const float t = cf * iv[l];
            const float val = mn[l] + t;
            const float prod = qv[l] * val;
            total = total + prod;
        }
    }
    return total;
}

constexpr int kSqAhead = 4;  // 16-byte code groups in flight per lane

// one row's score from its tile pieces: L2 = the 16 lane accumulators of sq8u_l2_batch + tail,
// DOT = the sequential sum above
template <bool DOT>
__device__ __forceinline__ float sq8_row_score(const uint4 *__restrict__ tp, int groups, int full, int tail,
                                               const float *__restrict__ qv, const float *__restrict__ mins,
                                               const float *__restrict__ inv)
{
    float acc[16];
#pragma unroll
    for (int l = 0; l < 16; l++) acc[l] = 0.0f;
    float run = 0.0f;
    // kSqAhead groups of codes in flight per lane (one ahead left the wave waiting on HBM every
    // 64 VALU instructions); addresses past the row's last group are clamped to it
    uint4 ring[kSqAhead];
    const int glast = groups - 1;
#pragma unroll
    for (int a = 0; a < kSqAhead; a++) ring[a] = load_stream(tp + (a < glast ? a : glast) * 64);
    for (int g0 = 0; g0 < full; g0 += kSqAhead) {
#pragma unroll
        for (int a = 0; a < kSqAhead; a++) {
            const int g = g0 + a;
            const uint4 c = ring[a];
            const int gn = g + kSqAhead;
            ring[a] = load_stream(tp + (gn < glast ? gn : glast) * 64);
            if (g < full) {
                if (DOT)
                    run = sq8_dot16(run, c, 16, qv + g * 16, mins + g * 16, inv + g * 16);
                else
                    sq8_block16(acc, c, qv + g * 16, mins + g * 16, inv + g * 16);
            }
        }
    }
    if (DOT) {
        if (tail) run = sq8_dot16(run, tp[full * 64], tail, qv + full * 16, mins + full * 16, inv + full * 16);
        return run;
    }
    float total = reduce16_regs(acc);
    if (tail) total = sq8_tail(total, tp[full * 64], tail, qv + full * 16, mins + full * 16, inv + full * 16);
    return total;
}

// The same with the ring carried ACROSS tiles (dim % 64 == 0: no tail group, whole ring rounds): the last round of a
// tile refills the ring with the first groups of the wave's NEXT tile, so a tile no longer starts with kSqAhead loads
// and an exposed HBM round trip (~2 us of the ~33 us a wave spends on a tile: 6.05 -> 6.4 TB/s at 4M x 768).
// `ring` arrives holding groups 0 .. kSqAhead-1 of this tile and leaves holding those of `tp_next`.
template <bool DOT>
__device__ __forceinline__ float sq8_row_score_stream(const uint4 *__restrict__ tp, const uint4 *__restrict__ tp_next, int full,
                                                      uint4 (&ring)[kSqAhead], const float *__restrict__ qv,
                                                      const float *__restrict__ mins, const float *__restrict__ inv)
{
    float acc[16];
#pragma unroll
    for (int l = 0; l < 16; l++) acc[l] = 0.0f;
    float run = 0.0f;
    for (int g0 = 0; g0 < full; g0 += kSqAhead) {
        const uint4 *src = g0 + kSqAhead < full ? tp + (g0 + kSqAhead) * 64 : tp_next;  // (uniform)
#pragma unroll
        for (int a = 0; a < kSqAhead; a++) {
            const int g = g0 + a;
            const uint4 c = ring[a];
            ring[a] = load_stream(src + a * 64);
            if (DOT)
                run = sq8_dot16(run, c, 16, qv + g * 16, mins + g * 16, inv + g * 16);
            else
                sq8_block16(acc, c, qv + g * 16, mins + g * 16, inv + g * 16);
        }
    }
    return DOT ? run : reduce16_regs(acc);
}

}  // namespace vg
