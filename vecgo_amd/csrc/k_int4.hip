// k_int4.hip — the 4-bit quantizer: quantization.Int4Quantizer (internal/quantization/int4.go,
// internal/simd/src/int4_avx512.c) and the INT4 codes of a DiskANN index.
#include <algorithm>
#include <type_traits>

#include "vg_device.hpp"
#include "vg_int4_plan.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"

namespace vg {

// stage 2 of Train (int4.go:52-61; stage 1 is the SQ8 Train's, launch_dim_minmax): diff = max - min, 0 -> 1; then BuildInt4LookupTable
// (kernels.go:94-103): table[d*16+q] = (float32(q)/15.0)*diff + min, three rounded operations
__global__ void int4_finish_kernel(const float *__restrict__ pmin, const float *__restrict__ pmax, int chunks,
                                   int dim, float *__restrict__ mins, float *__restrict__ diff)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= dim) return;
    float mn = kF32Max, mx = -kF32Max;
    for (int c = 0; c < chunks; c++) {
        const float a = pmin[static_cast<int64_t>(c) * dim + d], b = pmax[static_cast<int64_t>(c) * dim + d];
        if (a < mn) mn = a;
        if (b > mx) mx = b;
    }
    const float df = mx - mn;
    mins[d] = mn;
    diff[d] = df == 0.0f ? 1.0f : df;
}

__global__ void int4_table_kernel(const float *__restrict__ mins, const float *__restrict__ diff, int dim,
                                  float *__restrict__ table)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= dim * 16) return;
    const int d = t >> 4, q = t & 15;
    const float a = static_cast<float>(q) / 15.0f;
    const float b = a * diff[d];
    table[t] = b + mins[d];
}

__device__ __forceinline__ uint32_t int4_quant(float v, float mn, float df)
{
    float norm = (v - mn) / df;  // int4.go:75-81
    if (norm < 0.0f)
        norm = 0.0f;
    else if (norm > 1.0f)
        norm = 1.0f;
    return static_cast<uint32_t>(round(static_cast<double>(norm) * 15.0));  // math.Round(float64(norm) * 15)
}

// Encode (int4.go:65-105): thread per output byte
__global__ void int4_encode_kernel(const float *__restrict__ v, int64_t n, int dim, const float *__restrict__ mins,
                                   const float *__restrict__ diff, uint8_t *__restrict__ out)
{
    const int cs = (dim + 1) / 2;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= n * cs) return;
    const int64_t row = t / cs;
    const int i = static_cast<int>(t % cs) * 2;
    const float *x = v + row * dim;
    const uint32_t q1 = int4_quant(x[i], mins[i], diff[i]);
    const uint32_t q2 = i + 1 < dim ? int4_quant(x[i + 1], mins[i + 1], diff[i + 1]) : 0u;
    out[t] = static_cast<uint8_t>((q1 << 4) | (q2 & 0x0Fu));
}

// Decode (int4.go:108-130): float32(q)/15.0*diff + min, left to right
__global__ void int4_decode_kernel(const uint8_t *__restrict__ codes, int64_t n, int dim,
                                   const float *__restrict__ mins, const float *__restrict__ diff,
                                   float *__restrict__ out)
{
    const int cs = (dim + 1) / 2;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= n * dim) return;
    const int64_t row = t / dim;
    const int i = static_cast<int>(t % dim);
    const uint8_t b = codes[row * cs + i / 2];
    const float a = static_cast<float>((i & 1) ? (b & 0x0F) : (b >> 4)) / 15.0f;
    const float c = a * diff[i];
    out[t] = c + mins[i];
}

// dim % 8 == 0, aligned buffers: a thread owns eight consecutive dimensions = four code bytes (see sq8_encode4_kernel, k_sq8.hip)
__global__ __launch_bounds__(256) void int4_encode8_kernel(const float *__restrict__ v, int64_t n, int dim,
                                                           const float *__restrict__ mins, const float *__restrict__ diff,
                                                           uint8_t *__restrict__ out, int rpt)
{
    const int cg = blockIdx.x * blockDim.x + threadIdx.x;
    if (cg * 8 >= dim) return;
    const float4 mn0 = *reinterpret_cast<const float4 *>(mins + cg * 8), mn1 = *reinterpret_cast<const float4 *>(mins + cg * 8 + 4),
                 df0 = *reinterpret_cast<const float4 *>(diff + cg * 8), df1 = *reinterpret_cast<const float4 *>(diff + cg * 8 + 4);
    const int cs = dim >> 1;
    const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpt;
    for (int64_t row = r0; row < r0 + rpt && row < n; row++) {
        const float4 a = *reinterpret_cast<const float4 *>(v + row * dim + cg * 8), b = *reinterpret_cast<const float4 *>(v + row * dim + cg * 8 + 4);
        const uint32_t b0 = (int4_quant(a.x, mn0.x, df0.x) << 4) | (int4_quant(a.y, mn0.y, df0.y) & 0x0Fu);
        const uint32_t b1 = (int4_quant(a.z, mn0.z, df0.z) << 4) | (int4_quant(a.w, mn0.w, df0.w) & 0x0Fu);
        const uint32_t b2 = (int4_quant(b.x, mn1.x, df1.x) << 4) | (int4_quant(b.y, mn1.y, df1.y) & 0x0Fu);
        const uint32_t b3 = (int4_quant(b.z, mn1.z, df1.z) << 4) | (int4_quant(b.w, mn1.w, df1.w) & 0x0Fu);
        *reinterpret_cast<uint32_t *>(out + row * cs + cg * 4) = (b0 & 0xFFu) | ((b1 & 0xFFu) << 8) | ((b2 & 0xFFu) << 16) | (b3 << 24);
    }
}
__global__ __launch_bounds__(256) void int4_decode8_kernel(const uint8_t *__restrict__ codes, int64_t n, int dim,
                                                           const float *__restrict__ mins, const float *__restrict__ diff,
                                                           float *__restrict__ out, int rpt)
{
    const int cg = blockIdx.x * blockDim.x + threadIdx.x;
    if (cg * 8 >= dim) return;
    const float4 mn0 = *reinterpret_cast<const float4 *>(mins + cg * 8), mn1 = *reinterpret_cast<const float4 *>(mins + cg * 8 + 4),
                 df0 = *reinterpret_cast<const float4 *>(diff + cg * 8), df1 = *reinterpret_cast<const float4 *>(diff + cg * 8 + 4);
    const int cs = dim >> 1;
    const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpt;
    auto dec = [](uint32_t q, float df, float mn) -> float {
        const float a = static_cast<float>(q) / 15.0f;
        const float c = a * df;
        return c + mn;
    };
    for (int64_t row = r0; row < r0 + rpt && row < n; row++) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(codes + row * cs + cg * 4);
        float4 o0, o1;
        o0.x = dec((w >> 4) & 0xFu, df0.x, mn0.x);
        o0.y = dec(w & 0xFu, df0.y, mn0.y);
        o0.z = dec((w >> 12) & 0xFu, df0.z, mn0.z);
        o0.w = dec((w >> 8) & 0xFu, df0.w, mn0.w);
        o1.x = dec((w >> 20) & 0xFu, df1.x, mn1.x);
        o1.y = dec((w >> 16) & 0xFu, df1.y, mn1.y);
        o1.z = dec(w >> 28, df1.z, mn1.z);
        o1.w = dec((w >> 24) & 0xFu, df1.w, mn1.w);
        *reinterpret_cast<float4 *>(out + row * dim + cg * 8) = o0;
        *reinterpret_cast<float4 *>(out + row * dim + cg * 8 + 4) = o1;
    }
}

__device__ __forceinline__ float int4_nib(const uint8_t *code, int j)
{
    const uint8_t b = code[j >> 1];
    return static_cast<float>((j & 1) ? (b & 0x0F) : (b >> 4));
}

// int4L2DistanceBatchAvx512 (int4_avx512.c:191-299), lane per row: 64-element blocks feed sub-blocks
// 0,1 into sum1 and 2,3 into sum2, 32-element blocks both into sum1; dq = fma(f * (1/15), diff, min)
__global__ __launch_bounds__(256) void int4_l2_batch_kernel(const float *__restrict__ query,
                                                            const uint8_t *__restrict__ codes, int64_t n, int dim,
                                                            const float *__restrict__ mins,
                                                            const float *__restrict__ diff, float *__restrict__ out)
{
    const int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint8_t *code = codes + row * ((dim + 1) / 2);
    const float sc = __uint_as_float(0x3d888889u);  // int4_avx512.c:35
    float s1[16], s2[16];
#pragma unroll
    for (int l = 0; l < 16; l++) s1[l] = s2[l] = 0.0f;
    auto block = [&](float (&acc)[16], int base) {
#pragma unroll
        for (int l = 0; l < 16; l++) {
            const int j = base + l;
            const float f = int4_nib(code, j) * sc;
            const float dq = __builtin_fmaf(f, diff[j], mins[j]);
            const float d = query[j] - dq;
            acc[l] = __builtin_fmaf(d, d, acc[l]);
        }
    };
    int i = 0;
    for (; i <= dim - 64; i += 64) {
        block(s1, i);
        block(s1, i + 16);
        block(s2, i + 32);
        block(s2, i + 48);
    }
    for (; i <= dim - 32; i += 32) {
        block(s1, i);
        block(s1, i + 16);
    }
#pragma unroll
    for (int l = 0; l < 16; l++) s1[l] = s1[l] + s2[l];
    float total = reduce16_regs(s1);
    for (; i < dim; i++) {
        const float f = int4_nib(code, i) * sc;
        const float v = __builtin_fmaf(f, diff[i], mins[i]);
        const float d = query[i] - v;
        total = __builtin_fmaf(d, d, total);
    }
    out[row] = total;
}

__global__ __launch_bounds__(256) void int4_l2_precomputed_kernel(const float *__restrict__ query,
                                                                  const uint8_t *__restrict__ codes, int64_t n,
                                                                  int dim, const float *__restrict__ table,
                                                                  float *__restrict__ out)
{
    const int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (row >= n) return;
    out[row] = int4_l2_precomputed(query, codes + row * ((dim + 1) / 2), dim, table);
}

// Both distances as a streaming scan (dim % 64 == 0): the lane-per-row kernels above read their rows 16 bytes at a
// time at a dim/2-byte stride (64 lines per wave-instruction; 1.0 / 2.2 TB/s of codes at dim 768) and look every value
// up in a 48 KiB table.  Here a wave takes 64 rows: 128-byte pieces of them (256 dimensions) arrive as whole lines
// (8 lanes per row) and are turned through the wave's LDS (row stride 144 bytes = 16 x 9: the 16 lanes of a
// ds_read_b128 group never share a bank slot), each lane then walks ITS row; a code byte becomes its two values by ONE
// read of a 256-entry pair table in LDS (PRE: float(v) / 15, the table's own factor — int4.go:152-163; batch order:
// float(v) * 0x3d888889 — int4_avx512.c:35), the two values of a byte are neighbouring AVX-512 lanes, so every step is
// one packed-fp32 instruction on the pair with scalar-loaded diff / min / query: 2 - 2.5 vector instructions per
// dimension.  Accumulators and their order are the kernels' above: PRE — both 16-element halves of a 32-block into
// sum[]; batch order — sub-blocks 0, 1 of a 64-block into s1, 2, 3 into s2, s1 += s2 at the end.
template <bool PRE>
__global__ __launch_bounds__(kI4Waves * 64) void int4_scan_kernel(const float *__restrict__ query,
                                                                  const uint8_t *__restrict__ codes, int64_t n, int dim,
                                                                  const float *__restrict__ mins,
                                                                  const float *__restrict__ diff, float *__restrict__ out)
{
    __shared__ vg_f2v pairs[256];
    __shared__ __attribute__((aligned(16))) unsigned char stage_all[kI4Waves][64 * kI4Stride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const float sc = __uint_as_float(0x3d888889u);
        const int b = tid;  // 256 threads, 256 entries
        vg_f2v a;
        a.x = PRE ? static_cast<float>(b >> 4) / 15.0f : static_cast<float>(b >> 4) * sc;
        a.y = PRE ? static_cast<float>(b & 15) / 15.0f : static_cast<float>(b & 15) * sc;
        pairs[b] = a;
    }
    __syncthreads();
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * kI4Waves + wave;
    const int64_t row0 = tile * 64;
    if (row0 >= n) return;
    unsigned char *stage = stage_all[wave];
    const int row_bytes = dim >> 1;
    vg_f2v s1[8], s2[8];
#pragma unroll
    for (int p = 0; p < 8; p++) s1[p] = s2[p] = vg_f2v{0.0f, 0.0f};
    // one 32-element block (16 code bytes, `piece` of the staged row piece) into the accumulators
    auto block32 = [&](int cb0, int piece, auto second_c) {
        const uint4 c = *reinterpret_cast<const uint4 *>(stage + lane * kI4Stride + piece * 16);
        const uint32_t w[4] = {c.x, c.y, c.z, c.w};
        const int j0 = (cb0 + piece * 16) * 2;    // first dimension of the block
        constexpr bool second = !PRE && decltype(second_c)::value;  // batch order: sub-blocks 2, 3 of the 64-block
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const uint32_t byte = (w[b >> 2] >> (8 * (b & 3))) & 0xFFu;
            const int j = j0 + 2 * b;
            const vg_f2v a = pairs[byte];
            const vg_f2v df = *reinterpret_cast<const vg_f2v *>(diff + j);
            const vg_f2v mn = *reinterpret_cast<const vg_f2v *>(mins + j);
            const vg_f2v qq = *reinterpret_cast<const vg_f2v *>(query + j);
            vg_f2v t;
            if (PRE) {
                t = a * df;
                t = t + mn;
            } else {
                t = __builtin_elementwise_fma(a, df, mn);
            }
            const vg_f2v d = qq - t;
            if (second)
                s2[b & 7] = __builtin_elementwise_fma(d, d, s2[b & 7]);
            else
                s1[b & 7] = __builtin_elementwise_fma(d, d, s1[b & 7]);
        }
    };
    // rows past n re-read row n - 1 (their result is not stored); loads are unguarded (a guarded load makes hipcc
    // wait for the previous one at the join)
    if (int4_whole_pieces(row_bytes)) {
        // whole 128-byte pieces: 8 lanes per row, the next piece's lines in flight while this one is scored
        const int r = lane >> 3, part = lane & 7;
        const uint8_t *src[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int64_t row = row0 + r + 8 * k < n ? row0 + r + 8 * k : n - 1;
            src[k] = codes + row * row_bytes + part * 16;
        }
        uint4 u[8];
#pragma unroll
        for (int k = 0; k < 8; k++) u[k] = load_stream(reinterpret_cast<const uint4 *>(src[k]));
        for (int cb0 = 0; cb0 < row_bytes; cb0 += 128) {
#pragma unroll
            for (int k = 0; k < 8; k++) *reinterpret_cast<uint4 *>(stage + (r + 8 * k) * kI4Stride + part * 16) = u[k];
            const int nxt = cb0 + 128 < row_bytes ? cb0 + 128 : cb0;  // (the last piece again: unused)
#pragma unroll
            for (int k = 0; k < 8; k++) u[k] = load_stream(reinterpret_cast<const uint4 *>(src[k] + nxt));
            for (int piece = 0; piece < 8; piece += 2) {
                block32(cb0, piece, std::false_type{});
                block32(cb0, piece + 1, std::true_type{});
            }
        }
    } else {
        for (int cb0 = 0; cb0 < row_bytes; cb0 += 128) {
            const int cb = row_bytes - cb0 < 128 ? row_bytes - cb0 : 128;  // bytes of this piece (a multiple of 32)
            const int per_row = cb >> 4;                                    // 16-byte units per row
            const int units = 64 * per_row;
            uint4 u[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int e = lane + 64 * k < units ? lane + 64 * k : units - 1;
                const int r = e / per_row, part = e - r * per_row;
                const int64_t row = row0 + r < n ? row0 + r : n - 1;
                u[k] = load_stream(reinterpret_cast<const uint4 *>(codes + row * row_bytes + cb0 + part * 16));
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int e = lane + 64 * k;
                if (e < units) {
                    const int r = e / per_row, part = e - r * per_row;
                    *reinterpret_cast<uint4 *>(stage + r * kI4Stride + part * 16) = u[k];
                }
            }
            for (int piece = 0; piece < per_row; piece += 2) {  // per_row is even (dim % 64 == 0)
                block32(cb0, piece, std::false_type{});
                block32(cb0, piece + 1, std::true_type{});
            }
        }
    }
    float s16[16];
#pragma unroll
    for (int p = 0; p < 8; p++) {
        const vg_f2v v = PRE ? s1[p] : s1[p] + s2[p];
        s16[2 * p] = v.x;
        s16[2 * p + 1] = v.y;
    }
    const float total = reduce16_regs(s16);
    if (row0 + lane < n) out[row0 + lane] = total;
}

// The same scan with the lookups free of bank conflicts (dim <= 1024): the pair table above puts a wave's 64 random
// bytes on 32 bank slots — 62 % of its LDS cycles were conflicts and the LDS array was 89 % busy (3.65 TB/s of codes).
// Here the workgroup (12 waves, one per CU, persistent over the tiles) builds the quantizer's own dim x 16 value table
// in LDS (48 KiB at dim 768; PRE: float(v) / 15 * diff + min as BuildInt4LookupTable does; batch order:
// fma(float(v) * 0x3d888889, diff, min)): the 64 lanes of a lookup share the dimension, so they touch at most 16
// consecutive dwords — distinct banks or the same address.  A lookup's address is ONE v_perm_b32 (byte k of the
// pre-masked nibbles under the block's base; the dimension's offset is the instruction's immediate), a dimension
// costs 2 vector instructions (the table holds query[j] - value: a launch serves one query) and 2 LDS cycles per wave
// instead of ~3.5.  Rows are staged a whole 128-byte line at a time (stride 144 = 16 x 9; 12 waves beside the table:
// with 64-byte pieces and 16 waves the second half of a line was requested a step after the first and had often left
// L2 by then — the lines in flight on an XCD are about its 4 MiB — 1.34x the codes' bytes crossed the fabric).
// (the lookups are issued in inline asm, eight at a time — the four code bytes of one dword — and a group is retired by
// a COUNTED wait while the next group's eight are in flight: hipcc re-used one register pair per lookup and waited out
// every LDS round trip.  hipcc does not track asm loads: every value is an in/out operand of the wait statement, so no
// consumer can be scheduled above it.  LDS operations retire in order, scalar loads do not: nothing in the loop may
// issue one, which is one reason the table holds query[j] - value and not the value)
template <int OFF>
__device__ __forceinline__ float i4_lds_read(uint32_t addr)
{
    float v;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
struct I4Vals8 {
    float v[8];  // (hi, lo) of code bytes 4 WI .. 4 WI + 3
};
template <int N>
__device__ __forceinline__ void i4_lds_wait(I4Vals8 &x)
{
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(x.v[0]), "+v"(x.v[1]), "+v"(x.v[2]), "+v"(x.v[3]), "+v"(x.v[4]), "+v"(x.v[5]), "+v"(x.v[6]), "+v"(x.v[7])
                 : "n"(N));
}
template <int WI>
__device__ __forceinline__ void i4_issue_word(I4Vals8 &x, uint32_t w, uint32_t base)
{
    const uint32_t hi4 = (w >> 2) & 0x3C3C3C3Cu;  // byte k: 4 * high nibble of code byte 4 WI + k
    const uint32_t lo4 = (w << 2) & 0x3C3C3C3Cu;  //         4 * low nibble
#define VG_I4_ONE(K)                                                                                              \
    x.v[2 * K] = i4_lds_read<(2 * (4 * WI + K)) * 64>(__builtin_amdgcn_perm(base, hi4, 0x07060500u | K));         \
    x.v[2 * K + 1] = i4_lds_read<(2 * (4 * WI + K) + 1) * 64>(__builtin_amdgcn_perm(base, lo4, 0x07060500u | K));
    VG_I4_ONE(0)
    VG_I4_ONE(1)
    VG_I4_ONE(2)
    VG_I4_ONE(3)
#undef VG_I4_ONE
}

#ifdef VG_I4_TIMING  // stage probe (tools/build_variant.sh): s_memtime per phase, totals written over out[] by lane 0
#define VG_I4_T(var) const int64_t var = static_cast<int64_t>(__builtin_readcyclecounter())
#define VG_I4_TACC(acc, a, b) (acc) += (b) - (a)
#else
#define VG_I4_T(var)
#define VG_I4_TACC(acc, a, b)
#endif

// the 16 code bytes of a 32-element block, read from the wave's staging buffer under the same in-order accounting as
// the lookups ("memory": the staging writes before it stay before it, the next piece's writes stay after the last one)
typedef uint32_t i4_u4 __attribute__((ext_vector_type(4)));  // one register tuple as an asm operand: no sub-register copies
__device__ __forceinline__ i4_u4 i4_lds_read_block(uint32_t addr)
{
    i4_u4 c;
    asm volatile("ds_read_b128 %0, %1" : "=v"(c) : "v"(addr) : "memory");
    return c;
}
template <int N>
__device__ __forceinline__ void i4_lds_wait_c(I4Vals8 &x, i4_u4 &c)
{
    asm volatile("s_waitcnt lgkmcnt(%9)"
                 : "+v"(x.v[0]), "+v"(x.v[1]), "+v"(x.v[2]), "+v"(x.v[3]), "+v"(x.v[4]), "+v"(x.v[5]), "+v"(x.v[6]), "+v"(x.v[7]),
                   "+v"(c)
                 : "n"(N));
}
__device__ __forceinline__ void i4_lds_drain(i4_u4 &c)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(c) : : "memory");
}

// r04: the lookups of a whole 128-byte piece (8 blocks x 4 words x 8 lookups) run as ONE software pipeline — two words
// (16 lookups) in flight across block boundaries, the next block's 16 code bytes requested (asm, same queue) while the
// current block's second word is still out — where r03 drained the queue at the end of every 32-element block and then
// waited out the read of the next block's bytes: two LDS round trips per 32 dimensions with nothing of this wave in
// flight (stage probe -DVG_I4_TIMING: 83 % of a wave's time is the lookup phase, and its rate was that of a loop with
// those bubbles, not that of the vector ALU: tools/ubench/lds_valu_overlap.hip).  LDS operations of a wave return in
// order, so "at most N outstanding" names exactly which word is back: per block the counted waits are 9, 9, 8, 8 (the
// 9s have the next block's ds_read_b128 behind them).  The rows' addresses are a per-tile scalar base + a per-lane
// 32-bit offset (global_load saddr form): no 64-bit pointer arithmetic or selects per piece (r03: 32 of the 544 vector
// instructions of a piece).  Arithmetic and its order are unchanged: block b, words 0..3, accumulator (4 wi + k) & 7.
template <bool PRE>
__global__ __launch_bounds__(kI4TabWaves * 64) void int4_scan_tab_kernel(const float *__restrict__ query,
                                                                         const uint8_t *__restrict__ codes, int64_t n, int dim,
                                                                         const float *__restrict__ mins,
                                                                         const float *__restrict__ diff, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char i4smem[];
    float *table = reinterpret_cast<float *>(i4smem);  // [dim][16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // a scalar: the tile's base address lives in SGPRs
    unsigned char *stage = i4smem + static_cast<size_t>(dim) * 64 + wave * (64 * kI4TabStride);
    const int waves = blockDim.x >> 6;  // 12, fewer when the table leaves less room (dim 1024: 10)
    for (int e = tid; e < dim * 16; e += blockDim.x) {
        const int d = e >> 4, v = e & 15;
        float t;
        if (PRE) {
            const float a = static_cast<float>(v) / 15.0f;  // int4_table_kernel
            const float b = a * diff[d];
            t = b + mins[d];
        } else {
            const float f = static_cast<float>(v) * __uint_as_float(0x3d888889u);  // int4_l2_batch_kernel
            t = __builtin_fmaf(f, diff[d], mins[d]);
        }
        table[e] = query[d] - t;  // the difference the kernels square: one query per launch
    }
    __syncthreads();
    const int row_bytes = dim >> 1;
    const int64_t n_tiles = (n + 63) / 64;
    const int r = lane >> 3, part = lane & 7;  // staging: 8 lanes per row (one 128-byte line), 8 rows per load
    const int64_t tile_step = static_cast<int64_t>(gridDim.x) * waves;
    int64_t tile = static_cast<int64_t>(blockIdx.x) * waves + wave;
    if (tile >= n_tiles) return;
    // the table is the first thing in LDS: its real address (0 unless something static ever lands in this kernel's LDS)
    // goes into every lookup's base, and must leave the low 11 bits of a block's base free for the nibble byte
    const uint32_t table_lds = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(table));
    const uint32_t stage_rd = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(stage)) + lane * kI4TabStride;
    if ((table_lds & 2047u) != 0) __builtin_trap();
    // per-lane byte offsets of the 8 rows this lane helps to load, relative to the tile's first row; rows past n
    // (last tile only) read row n - 1 again and are not stored
    auto offsets = [&](int64_t t, uint32_t (&vo)[8]) {
        const int64_t left = n - t * 64;  // rows in the tile
        const uint32_t lim = left >= 64 ? 63u : static_cast<uint32_t>(left - 1);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t rr = static_cast<uint32_t>(r + 8 * k);
            vo[k] = (rr < lim ? rr : lim) * static_cast<uint32_t>(row_bytes) + static_cast<uint32_t>(part * 16);
        }
    };
    uint32_t vo[8];
    offsets(tile, vo);
    const uint8_t *tbase = codes + tile * 64 * row_bytes;  // uniform
#define VG_I4_ROWS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define VG_I4_DECL(K) uint4 u##K = load_stream(reinterpret_cast<const uint4 *>(tbase + vo[K]));
    VG_I4_ROWS(VG_I4_DECL)
#undef VG_I4_DECL
    unsigned char *wr = stage + r * kI4TabStride + part * 16;
#ifdef VG_I4_TIMING
    int64_t t_vm = 0, t_ld = 0, t_look = 0, t_tiles = 0;
    const int64_t t_begin = static_cast<int64_t>(__builtin_readcyclecounter());
#endif
    for (; tile < n_tiles; tile += tile_step) {
#ifdef VG_I4_TIMING
        t_tiles++;
#endif
        const int64_t row0 = tile * 64;
        // the wave's next tile (its first piece is requested while this tile's last one is scored); none: this tile again
        const int64_t tnext = tile + tile_step < n_tiles ? tile + tile_step : tile;
        const uint8_t *nbase = codes + tnext * 64 * row_bytes;
        uint32_t von[8];
        offsets(tnext, von);
        vg_f2v s1[8], s2[8];
#pragma unroll
        for (int p = 0; p < 8; p++) s1[p] = s2[p] = vg_f2v{0.0f, 0.0f};
        for (int cb0 = 0; cb0 < row_bytes; cb0 += 128) {
            VG_I4_T(tA);
#define VG_I4_PUT(K) *reinterpret_cast<uint4 *>(wr + 8 * K * kI4TabStride) = u##K;
            VG_I4_ROWS(VG_I4_PUT)
#undef VG_I4_PUT
            VG_I4_T(tB);
            VG_I4_TACC(t_vm, tA, tB);
            i4_u4 c = i4_lds_read_block(stage_rd);
            {   // the next piece of this tile, or the first piece of the wave's next tile: a scalar base and a per-lane
                // 32-bit offset either way (uniform selects; a branch here became per-lane 64-bit pointers again)
                const bool more = cb0 + 128 < row_bytes;
                const uint8_t *pb = more ? tbase + cb0 + 128 : nbase;
#define VG_I4_GET(K) u##K = load_stream(reinterpret_cast<const uint4 *>(pb + (more ? vo[K] : von[K])));
                VG_I4_ROWS(VG_I4_GET)
#undef VG_I4_GET
            }
            i4_lds_drain(c);  // the staging writes and the first block's bytes
            VG_I4_T(tC);
            VG_I4_TACC(t_ld, tB, tC);
            const uint32_t pbase = table_lds + static_cast<uint32_t>(cb0) * 128u;  // table row of the piece's first dimension: j * 64 bytes
            I4Vals8 va, vb;
            i4_issue_word<0>(va, c.x, pbase);
            i4_issue_word<1>(vb, c.y, pbase);
#pragma unroll
            for (int blk = 0; blk < 8; blk++) {
                const uint32_t base = pbase + static_cast<uint32_t>(blk) * 2048u;  // 32 dimensions x 64 bytes
                vg_f2v *acc = (!PRE && (blk & 1)) ? s2 : s1;
                auto take = [&](const I4Vals8 &x, int wi) {  // code bytes 4 wi .. 4 wi + 3: accumulator pairs (4 wi + k) & 7
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const vg_f2v d = {x.v[2 * k], x.v[2 * k + 1]};
                        acc[(4 * wi + k) & 7] = __builtin_elementwise_fma(d, d, acc[(4 * wi + k) & 7]);
                    }
                };
                i4_u4 cn = c;
                if (blk < 7) {
                    cn = i4_lds_read_block(stage_rd + (blk + 1) * 16);
                    i4_lds_wait<9>(va);  // behind word 0: word 1 and the next block's bytes
                    take(va, 0);
                    i4_issue_word<2>(va, c.z, base);
                    i4_lds_wait<9>(vb);  // behind word 1: the bytes and word 2
                    take(vb, 1);
                    i4_issue_word<3>(vb, c.w, base);
                    i4_lds_wait_c<8>(va, cn);  // behind word 2: word 3 — the next block's bytes are older, so they are back
                    take(va, 2);
                    i4_issue_word<0>(va, cn.x, base + 2048u);
                    i4_lds_wait<8>(vb);
                    take(vb, 3);
                    i4_issue_word<1>(vb, cn.y, base + 2048u);
                    c = cn;
                } else {
                    i4_lds_wait<8>(va);
                    take(va, 0);
                    i4_issue_word<2>(va, c.z, base);
                    i4_lds_wait<8>(vb);
                    take(vb, 1);
                    i4_issue_word<3>(vb, c.w, base);
                    i4_lds_wait<8>(va);
                    take(va, 2);
                    i4_lds_wait<0>(vb);
                    take(vb, 3);
                }
            }
            VG_I4_T(tD);
            VG_I4_TACC(t_look, tC, tD);
        }
        float s16[16];
#pragma unroll
        for (int p = 0; p < 8; p++) {
            const vg_f2v v = PRE ? s1[p] : s1[p] + s2[p];
            s16[2 * p] = v.x;
            s16[2 * p + 1] = v.y;
        }
        const float total = reduce16_regs(s16);
        if (row0 + lane < n) out[row0 + lane] = total;
        tbase = nbase;
#pragma unroll
        for (int k = 0; k < 8; k++) vo[k] = von[k];
    }
#undef VG_I4_ROWS
#ifdef VG_I4_TIMING
    if (lane == 0) {
        const int64_t t_all = static_cast<int64_t>(__builtin_readcyclecounter()) - t_begin;
        float *o = out + (static_cast<int64_t>(blockIdx.x) * waves + wave) * 8;
        o[0] = static_cast<float>(t_tiles);
        o[1] = static_cast<float>(t_all);
        o[2] = static_cast<float>(t_vm);
        o[3] = static_cast<float>(t_ld);
        o[4] = static_cast<float>(t_look);
    }
#endif
}

}  // namespace vg

// ---- C ABI --------------------------------------------------------------------------------------------
static int32_t int4_rebuild_table(vg_int4 *iq, hipStream_t st)
{
    VG_LAUNCH(vg::int4_table_kernel, dim3((iq->dim * 16 + 255) / 256), dim3(256), 0, st, iq->d_min, iq->d_diff,
              iq->dim, iq->d_table);
    VG_HIP(hipStreamSynchronize(st));
    iq->trained = true;
    return VG_OK;
}

VG_API int32_t vg_int4_create(vg_ctx *ctx, int32_t dim, vg_int4 **out)
{
    VG_CHECK(out, VG_ERR_INVALID_ARG, "vg_int4_create: out is NULL");
    *out = nullptr;
    VG_CHECK(ctx, VG_ERR_INVALID_ARG, "vg_int4_create: ctx is NULL");
    VG_CHECK(dim > 0, VG_ERR_INVALID_ARG, "vg_int4_create: dim must be positive");
    VG_HIP(hipSetDevice(ctx->device));
    vg_int4 *iq = new vg_int4;
    iq->ctx = ctx;
    iq->dim = dim;
    float *block = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&block), sizeof(float) * 18 * static_cast<size_t>(dim));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete iq;
        vg::set_error("vg_int4_create: hipMalloc failed: %s", hipGetErrorString(e));
        return VG_ERR_HIP;
    }
    iq->d_min = block;
    iq->d_diff = block + dim;
    iq->d_table = block + 2 * static_cast<size_t>(dim);
    *out = iq;
    return VG_OK;
}

VG_API int32_t vg_int4_destroy(vg_int4 *iq)
{
    if (!iq) return VG_OK;
    (void)hipSetDevice(iq->ctx->device);
    if (iq->d_min) (void)hipFree(iq->d_min);
    delete iq;
    return VG_OK;
}

VG_API int32_t vg_int4_is_trained(vg_int4 *iq) { return iq && iq->trained ? 1 : 0; }

VG_API int32_t vg_int4_train(vg_int4 *iq, const float *vectors, int64_t n, void *stream)
{
    VG_CHECK(iq, VG_ERR_INVALID_ARG, "vg_int4_train: NULL quantizer");
    VG_CHECK(n > 0 && vectors, VG_ERR_INVALID_ARG, "no vectors provided for training");  // int4.go:30-32
    VG_HIP(hipSetDevice(iq->ctx->device));
    hipStream_t st = vg::pick_stream(iq->ctx, stream);
    const int dim = iq->dim;
    vg::DevIn<float> v;
    VG_TRY(v.init(vectors, static_cast<size_t>(n) * dim, st));
    int chunks;
    vg::DevTmp<float> pmin, pmax;
    VG_TRY(vg::launch_dim_minmax(v.ptr, n, dim, pmin, pmax, chunks, st));
    VG_LAUNCH(vg::int4_finish_kernel, dim3((dim + 255) / 256), dim3(256), 0, st, pmin.ptr, pmax.ptr, chunks, dim, iq->d_min,
              iq->d_diff);
    return int4_rebuild_table(iq, st);
}

/* UnmarshalBinary (int4.go:190-219): min[dim], diff[dim] as stored, table rebuilt */
VG_API int32_t vg_int4_set_params(vg_int4 *iq, const float *min_val, const float *diff)
{
    VG_CHECK(iq, VG_ERR_INVALID_ARG, "vg_int4_set_params: NULL quantizer");
    VG_CHECK(min_val && diff, VG_ERR_INVALID_ARG, "vg_int4_set_params: NULL parameters");
    VG_HIP(hipSetDevice(iq->ctx->device));
    hipStream_t st = iq->ctx->stream;
    const size_t b = sizeof(float) * static_cast<size_t>(iq->dim);
    VG_HIP(hipMemcpyAsync(iq->d_min, min_val, b, hipMemcpyDefault, st));
    VG_HIP(hipMemcpyAsync(iq->d_diff, diff, b, hipMemcpyDefault, st));
    return int4_rebuild_table(iq, st);
}

VG_API int32_t vg_int4_get_params(vg_int4 *iq, float *min_val, float *diff, float *table)
{
    VG_CHECK(iq, VG_ERR_INVALID_ARG, "vg_int4_get_params: NULL quantizer");
    VG_CHECK(iq->trained, VG_ERR_NOT_TRAINED, "Int4Quantizer not trained");
    VG_HIP(hipSetDevice(iq->ctx->device));
    hipStream_t st = iq->ctx->stream;
    const size_t b = sizeof(float) * static_cast<size_t>(iq->dim);
    if (min_val) VG_HIP(hipMemcpyAsync(min_val, iq->d_min, b, hipMemcpyDefault, st));
    if (diff) VG_HIP(hipMemcpyAsync(diff, iq->d_diff, b, hipMemcpyDefault, st));
    if (table) VG_HIP(hipMemcpyAsync(table, iq->d_table, 16 * b, hipMemcpyDefault, st));
    VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}

VG_API int64_t vg_int4_code_bytes(int32_t dim) { return (static_cast<int64_t>(dim) + 1) / 2; }

VG_API int32_t vg_int4_encode(vg_int4 *iq, const float *vectors, int64_t n, uint8_t *codes, void *stream)
{
    VG_CHECK(iq, VG_ERR_INVALID_ARG, "vg_int4_encode: NULL quantizer");
    VG_CHECK(iq->trained, VG_ERR_NOT_TRAINED, "Int4Quantizer not trained");
    VG_CHECK(n >= 0, VG_ERR_INVALID_ARG, "vg_int4_encode: n < 0");
    if (n == 0) return VG_OK;
    VG_CHECK(vectors && codes, VG_ERR_INVALID_ARG, "vg_int4_encode: NULL buffer");
    VG_HIP(hipSetDevice(iq->ctx->device));
    hipStream_t st = vg::pick_stream(iq->ctx, stream);
    const int64_t cs = vg_int4_code_bytes(iq->dim);
    vg::DevIn<float> v;
    vg::DevOut<uint8_t> c;
    VG_TRY(v.init(vectors, static_cast<size_t>(n) * iq->dim, st, vg::kAnyAlign));
    VG_TRY(c.init(codes, static_cast<size_t>(n * cs), st, vg::kAnyAlign));
    const vg::RowWalk walk(n);
    if (iq->dim % 8 == 0 && vg::aligned16(v.ptr, c.ptr))
        VG_LAUNCH(vg::int4_encode8_kernel, dim3((iq->dim / 8 + 255) / 256, walk.blocks_y),
                  dim3(256), 0, st, v.ptr, n, iq->dim, iq->d_min, iq->d_diff, c.ptr, walk.rpt);
    else
        VG_LAUNCH(vg::int4_encode_kernel, dim3(static_cast<unsigned>((n * cs + 255) / 256)), dim3(256), 0, st, v.ptr, n,
                  iq->dim, iq->d_min, iq->d_diff, c.ptr);
    VG_TRY(c.finish());
    return VG_OK;
}

VG_API int32_t vg_int4_decode(vg_int4 *iq, const uint8_t *codes, int64_t n, float *out, void *stream)
{
    VG_CHECK(iq, VG_ERR_INVALID_ARG, "vg_int4_decode: NULL quantizer");
    VG_CHECK(iq->trained, VG_ERR_NOT_TRAINED, "Int4Quantizer not trained");
    VG_CHECK(n >= 0, VG_ERR_INVALID_ARG, "vg_int4_decode: n < 0");
    if (n == 0) return VG_OK;
    VG_CHECK(codes && out, VG_ERR_INVALID_ARG, "vg_int4_decode: NULL buffer");
    VG_HIP(hipSetDevice(iq->ctx->device));
    hipStream_t st = vg::pick_stream(iq->ctx, stream);
    const int64_t cs = vg_int4_code_bytes(iq->dim);
    vg::DevIn<uint8_t> c;
    vg::DevOut<float> o;
    VG_TRY(c.init(codes, static_cast<size_t>(n * cs), st, vg::kAnyAlign));
    VG_TRY(o.init(out, static_cast<size_t>(n) * iq->dim, st, vg::kAnyAlign));
    const vg::RowWalk walk(n);
    if (iq->dim % 8 == 0 && vg::aligned16(c.ptr, o.ptr))
        VG_LAUNCH(vg::int4_decode8_kernel, dim3((iq->dim / 8 + 255) / 256, walk.blocks_y),
                  dim3(256), 0, st, c.ptr, n, iq->dim, iq->d_min, iq->d_diff, o.ptr, walk.rpt);
    else
        VG_LAUNCH(vg::int4_decode_kernel, dim3(static_cast<unsigned>((n * iq->dim + 255) / 256)), dim3(256), 0, st, c.ptr, n,
                  iq->dim, iq->d_min, iq->d_diff, o.ptr);
    VG_TRY(o.finish());
    return VG_OK;
}

// precomputed = 0: L2DistanceBatch (int4.go:150-164, batch kernel order);
// precomputed = 1: L2Distance per code (int4.go:133-147, lookup-table kernel order)
VG_API int32_t vg_int4_l2_distance_batch(vg_int4 *iq, const float *query, const uint8_t *codes, int64_t n,
                                         int32_t precomputed, float *out, void *stream)
{
    VG_CHECK(iq, VG_ERR_INVALID_ARG, "vg_int4_l2_distance_batch: NULL quantizer");
    VG_CHECK(iq->trained, VG_ERR_NOT_TRAINED, "Int4Quantizer not trained");
    VG_CHECK(n >= 0, VG_ERR_INVALID_ARG, "vg_int4_l2_distance_batch: n < 0");
    if (n == 0) return VG_OK;
    VG_CHECK(query && codes && out, VG_ERR_INVALID_ARG, "vg_int4_l2_distance_batch: NULL buffer");
    VG_HIP(hipSetDevice(iq->ctx->device));
    hipStream_t st = vg::pick_stream(iq->ctx, stream);
    const int64_t cs = vg_int4_code_bytes(iq->dim);
    vg::DevIn<float> q;
    vg::DevIn<uint8_t> c;
    vg::DevOut<float> o;
    VG_TRY(q.init(query, static_cast<size_t>(iq->dim), st));
    VG_TRY(c.init(codes, static_cast<size_t>(n * cs), st, vg::kAnyAlign));
    VG_TRY(o.init(out, static_cast<size_t>(n), st));
    // the kernel and its launch shape: vg_int4_plan.hpp (the rule exists there alone; vg_int4_scan_plan shows it to a test)
    const vg::Int4ScanPlan plan = vg::int4_scan_plan(iq->dim, vg::aligned16(c.ptr), n, iq->ctx->compute_units, vg::hook(vg::kHookInt4SmallGrid));
    const dim3 grid(static_cast<unsigned>(plan.blocks)), block(plan.waves * 64);
    vg::ProfScope prof(iq->ctx, "int4_scan", st);
    if (plan.kernel == vg::kI4Tab) {
        auto kern = precomputed ? vg::int4_scan_tab_kernel<true> : vg::int4_scan_tab_kernel<false>;
        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(plan.lds)));
        VG_LAUNCH(kern, grid, block, static_cast<size_t>(plan.lds), st, q.ptr, c.ptr, n, iq->dim, iq->d_min, iq->d_diff, o.ptr);
    } else if (plan.kernel != vg::kI4Row && precomputed)
        VG_LAUNCH(vg::int4_scan_kernel<true>, grid, block, 0, st, q.ptr, c.ptr, n, iq->dim, iq->d_min, iq->d_diff, o.ptr);
    else if (plan.kernel != vg::kI4Row)
        VG_LAUNCH(vg::int4_scan_kernel<false>, grid, block, 0, st, q.ptr, c.ptr, n, iq->dim, iq->d_min, iq->d_diff, o.ptr);
    else if (precomputed)
        VG_LAUNCH(vg::int4_l2_precomputed_kernel, grid, block, 0, st, q.ptr, c.ptr, n, iq->dim, iq->d_table, o.ptr);
    else
        VG_LAUNCH(vg::int4_l2_batch_kernel, grid, block, 0, st, q.ptr, c.ptr, n, iq->dim, iq->d_min, iq->d_diff, o.ptr);
    VG_TRY(o.finish());
    return VG_OK;
}

// what vg_int4_l2_distance_batch would launch for n rows (read-only, nothing runs): plan[4] = {kernel (0 tab, 1 pair128,
// 2 pair_tail, 3 row: Int4ScanKernel), waves per workgroup, workgroups, dynamic LDS bytes}
VG_API int32_t vg_int4_scan_plan(vg_int4 *iq, int64_t n, int32_t codes_aligned16, int64_t *plan)
{
    VG_CHECK(iq && plan, VG_ERR_INVALID_ARG, "vg_int4_scan_plan: NULL quantizer or plan");
    VG_CHECK(n > 0, VG_ERR_INVALID_ARG, "vg_int4_scan_plan: n must be positive");
    const vg::Int4ScanPlan p = vg::int4_scan_plan(iq->dim, codes_aligned16 != 0, n, iq->ctx->compute_units, vg::hook(vg::kHookInt4SmallGrid));
    plan[0] = p.kernel;
    plan[1] = p.waves;
    plan[2] = p.blocks;
    plan[3] = p.lds;
    return VG_OK;
}

// INT4 codes of a DiskANN segment, n * ceil(dim/2) bytes row-major (diskann/segment.go:378-416):
// kept in that layout, the graph search reads them by node id
VG_API int32_t vg_index_set_int4_codes(vg_index *idx, vg_int4 *iq, const uint8_t *codes, void *stream)
{
    VG_CHECK(idx && iq, VG_ERR_INVALID_ARG, "vg_index_set_int4_codes: NULL index or quantizer");
    VG_CHECK(iq->trained, VG_ERR_NOT_TRAINED, "Int4Quantizer not trained");
    VG_CHECK(iq->dim == idx->dim, VG_ERR_DIM_MISMATCH, "dimension mismatch");
    VG_CHECK(idx->n == 0 || codes, VG_ERR_INVALID_ARG, "vg_index_set_int4_codes: codes is NULL");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    if (idx->d_int4_rows) {
        VG_HIP(hipStreamSynchronize(st));
        VG_HIP(hipFree(idx->d_int4_rows));
        idx->d_int4_rows = nullptr;
    }
    idx->int4_table = iq->d_table;
    idx->int4_min = iq->d_min;
    idx->int4_diff = iq->d_diff;
    if (idx->n == 0) return VG_OK;
    const size_t bytes = static_cast<size_t>(idx->n) * static_cast<size_t>(vg_int4_code_bytes(idx->dim));
    VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_int4_rows), bytes));
    VG_HIP(hipMemcpyAsync(idx->d_int4_rows, codes, bytes, hipMemcpyDefault, st));
    VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}
