// vg_int4_scan.hpp — the row loops of the streaming INT4 scans, shared by the distance kernels (k_int4.hip: the epilogue stores
// out[row]) and the exhaustive search (k_int4_search.hip: the epilogue offers the row's key to the wave's top-k).
//
// Epilogue (by reference; one per wave):
//   bool live_tile(int64_t tile, int lane)          wave-uniform: does any row of the 64-row tile take part?  A tile that does not
//                                                   is neither read nor scored (the search's batch mask; the distance scan: always)
//   void row(int64_t row0, int lane, float total)   lane `lane` of the wave holds the score of row row0 + lane (rows past n too:
//                                                   those re-read row n - 1 and the epilogue drops them)
#pragma once

#include <type_traits>

#include "vg_device.hpp"
#include "vg_int4_plan.hpp"

namespace vg {

// the distance scans' epilogue: out[row] = score
struct Int4StoreEpi {
    float *__restrict__ out;
    int64_t n;
    __device__ __forceinline__ constexpr bool live_tile(int64_t, int) const { return true; }
    __device__ __forceinline__ void row(int64_t row0, int lane, float total) const
    {
        if (row0 + lane < n) out[row0 + lane] = total;
    }
};

// Both distances as a streaming scan (dim % 64 == 0): the lane-per-row kernels read their rows 16 bytes at a
// time at a dim/2-byte stride (64 lines per wave-instruction; 1.0 / 2.2 TB/s of codes at dim 768) and look every value
// up in a 48 KiB table.  Here a wave takes 64 rows: 128-byte pieces of them (256 dimensions) arrive as whole lines
// (8 lanes per row) and are turned through the wave's LDS (row stride 144 bytes = 16 x 9: the 16 lanes of a
// ds_read_b128 group never share a bank slot), each lane then walks ITS row; a code byte becomes its two values by ONE
// read of a 256-entry pair table in LDS (PRE: float(v) / 15, the table's own factor — int4.go:152-163; batch order:
// float(v) * 0x3d888889 — int4_avx512.c:35), the two values of a byte are neighbouring AVX-512 lanes, so every step is
// one packed-fp32 instruction on the pair with scalar-loaded diff / min / query: 2 - 2.5 vector instructions per
// dimension.  Accumulators and their order are the lane-per-row kernels': PRE — both 16-element halves of a 32-block into
// sum[]; batch order — sub-blocks 0, 1 of a 64-block into s1, 2, 3 into s2, s1 += s2 at the end.
// the pair table of the kernel's order (256 threads, 256 entries; the caller's __syncthreads() follows)
template <bool PRE>
__device__ __forceinline__ void int4_scan_fill_pairs(vg_f2v *pairs, int tid)
{
    const float sc = __uint_as_float(0x3d888889u);
    const int b = tid;
    vg_f2v a;
    a.x = PRE ? static_cast<float>(b >> 4) / 15.0f : static_cast<float>(b >> 4) * sc;
    a.y = PRE ? static_cast<float>(b & 15) / 15.0f : static_cast<float>(b & 15) * sc;
    pairs[b] = a;
}
// one 64-row tile (rows row0 .. row0 + 63, row0 < n) by one wave; stage: the wave's 64 * kI4Stride bytes of LDS
template <bool PRE, class Epi>
__device__ __forceinline__ void int4_pair_tile(const float *__restrict__ query, const uint8_t *__restrict__ codes, int64_t n, int dim,
                                               const float *__restrict__ mins, const float *__restrict__ diff, const vg_f2v *pairs,
                                               unsigned char *stage, int lane, int64_t row0, Epi &epi)
{
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
    epi.row(row0, lane, reduce16_regs(s16));
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

#ifdef VG_I4_TIMING  // stage probe (tools/build_variant.sh): s_memtime per phase, totals written over timing_out[] by lane 0
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
//
// The whole workgroup calls (it builds the table and meets at a barrier); i4smem: the kernel's dynamic LDS, the table first (its
// address has the low 11 bits clear), then a staging buffer per wave.  The waves walk the live tiles wave, wave + step, ... of
// the workgroup's deal (tile = (trip * gridDim.x + blockIdx.x) * waves + wave).  A wave without a tile returns early.
template <bool PRE, class Epi>
__device__ __forceinline__ void int4_tab_scan(unsigned char *i4smem, const float *__restrict__ query, const uint8_t *__restrict__ codes,
                                              int64_t n, int dim, const float *__restrict__ mins, const float *__restrict__ diff,
                                              float *timing_out, Epi &epi)
{
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
    // the wave's first live tile at or after t
    auto live_from = [&](int64_t t) {
        while (t < n_tiles && !epi.live_tile(t, lane)) t += tile_step;
        return t;
    };
    int64_t tile = live_from(static_cast<int64_t>(blockIdx.x) * waves + wave);
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
    while (tile < n_tiles) {
#ifdef VG_I4_TIMING
        t_tiles++;
#endif
        const int64_t row0 = tile * 64;
        // the wave's next tile (its first piece is requested while this tile's last one is scored); none: this tile again
        const int64_t tfollow = live_from(tile + tile_step);
        const int64_t tnext = tfollow < n_tiles ? tfollow : tile;
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
        epi.row(row0, lane, reduce16_regs(s16));
        tbase = nbase;
#pragma unroll
        for (int k = 0; k < 8; k++) vo[k] = von[k];
        tile = tfollow;
    }
#undef VG_I4_ROWS
#ifdef VG_I4_TIMING
    if (lane == 0 && timing_out) {
        const int64_t t_all = static_cast<int64_t>(__builtin_readcyclecounter()) - t_begin;
        float *o = timing_out + (static_cast<int64_t>(blockIdx.x) * waves + wave) * 8;
        o[0] = static_cast<float>(t_tiles);
        o[1] = static_cast<float>(t_all);
        o[2] = static_cast<float>(t_vm);
        o[3] = static_cast<float>(t_ld);
        o[4] = static_cast<float>(t_look);
    }
#else
    (void)timing_out;
#endif
}

}  // namespace vg
