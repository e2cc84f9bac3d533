// vg_int4_small_gemm.hpp — the INT4 nomination's append GEMM for ONE query tile of up to 128 queries (flat_gemm_int4_small_kernel):
// bf16 queries (scaled by diff / 15) against the index's row-major INT4 codes, scoring in flat_gemm_int4_big_kernel's space,
//     s' = |x^|^2 - 2 (q o s).c',   c' = c - 8 exact in bfloat16 (int4_word_bf16), the image of q o s the only rounded operand.
// Kept in a header so that tools/ubench can time the same code; launched by k_int4_small.hip.
//
// The design is the small batch's own.  With a single query tile a row is consumed by exactly one wave, so staging rows in LDS
// buys nothing: a wave reads its rows' codes from global memory straight into the registers that feed v_mfma_f32_32x32x16_bf16,
// and LDS holds the queries' image alone.
//  * 256 threads as 1 x 4 waves; a row tile is 256 rows, wave w owns rows 64 w .. 64 w + 63 as two 32-row blocks; workgroups are
//    persistent over the row tiles (tile = blockIdx.x, + gridDim.x, ...).
//  * K is walked in SUPERSTEPS of 256 dimensions = 128 code bytes of a row = one cache line (rows start 16-byte aligned; at
//    dim % 256 == 0 every superstep of every row is a whole line).  The matrix instruction gives lane (r, h = lane >> 5) row r of the
//    block and the k-slice h: lane (r, h) loads the 64 bytes [64 h, 64 h + 64) of row r's line with four 16-byte loads — the two
//    lanes of a row take the line exactly once, in four back-to-back instructions, instead of a quarter of it in each of four
//    K steps that the L1 would have to bridge.  Load i (16 bytes = 32 dimensions) is word m = 0 .. 3 -> the four 8-element
//    k-slices of one 32-dimension block: matrix instruction (i, m) multiplies, in lane half h, dimensions
//        256 S + 32 (a h + i) + 8 m .. + 8        (a = 4: the loads a lane half owns in a whole superstep).
//    The query operand takes the SAME k-permutation per lane half — granule (i, m, h) of the image in LDS holds exactly those 8
//    dimensions — so every product pairs q_d with c'_d and the sum over a row is the dot product in another order (the argument
//    rabitq_nom_gemm_kernel makes for its tile).
//  * the last superstep of a row may be partial: `rest` 16-byte units (1 .. 7).  Lane half 0 owns the first a = (rest + 1) / 2 of
//    them, half 1 the others; only loads i < a are multiplied (wave-uniform).  At dim % 64 == 32 (rest odd) half 1's last unit
//    lies past the row: the lane re-reads unit 0 of the superstep — never a byte past the row — and its converted granule is
//    replaced by zeros; the image's granule there is zeros as well.
//  * the image is RESIDENT in LDS for the whole kernel, not streamed per K step.  Vector-memory operations retire in order: a
//    wait for a streamed piece of the image (an L2 hit) is a wait for every row load issued before it (HBM misses), so a stream
//    per K step would cut the row loads' flight time to one step and pay a barrier per step — and it would pull RB x 32 x 2
//    bytes per dimension from the L2 for every 256-row tile, twice the tile's code bytes at RB = 4.  Resident, the K loop has
//    no barrier and no LDS write at all: the row loads of the next superstep fly under the current one's matrix instructions
//    (also across tiles: the stream of supersteps does not drain at a tile's end).  What does not fit — 64 RB bytes per padded
//    dimension: RB = 4 from dim 608 on — is split ON THE HOST into launches of fewer 32-query blocks (launch_int4_small_gemm,
//    k_int4_small.hip): 97 .. 128 queries at dim 768 run as two launches of two blocks, a second pass over codes that the first
//    has partly left in the last-level cache.  Above dim 2496 not even one block fits and the batch keeps the scan.
//    Layout: granule ((slot 4 + m) 2 + h) QB + q, slot = 4 S + i, QB = 32 RB, 16 bytes each.  An operand read (fixed slot, m and
//    block) is 32 consecutive granules per lane half: every 16-lane pass of a ds_read_b128 covers 16 different 16-byte bank
//    groups.  Each read feeds the wave's two row blocks: 2 RB 4 matrix instructions for RB 4 ds_read_b128 per 32-dimension step.
//  * the epilogue is gemm_epilogue's append (vg_flat_gemm.hpp): score = fma(-2, acc, |x^|^2), compared with the query's threshold
//    (in LDS; -Inf for the padded queries of the last block: they never append), a returning atomic on the query's counter
//    parked until the tile's end, the key make_key(score, row) — the form Int4Row's verify pair reads.  Rows past n re-read the
//    last row and are never listed.
//  * row filters (vg_index_enable_int4_nomination's on & 4) are variants of their own, MASKED and BATCH template parameters: the
//    unfiltered instantiations are the code they were.
//    BATCH — one filter for all queries: a wave's 64 rows are 8 bytes of it.  A tile whose 8 bytes are zero is SKIPPED by its
//    wave: no code load, no matrix instruction, no epilogue (at 1 % kept rows about half of the 64-row tiles).  The wave has to
//    know the next tile it will compute while the current one's last superstep runs — that is when the next loads go out — so
//    the filter is read ahead, in WINDOWS of 8 of the wave's tiles: one vector load, lane l takes byte l & 7 of the wave's rows in
//    tile (8 w + (l >> 3)) of the workgroup's sequence, a ballot of "byte != 0" is the window's live tiles.  The window after the
//    current one is already in flight (issued when the current one was entered, a tile or more before its first use), so the
//    row loads never wait for a filter byte.  The epilogue's bit of row (j, r) comes out of the window's registers with one lane
//    shuffle per row block, at the tile's start, and stands beside `row < n`.  The waves of a workgroup skip independently: after
//    the image's barrier there is none.
//    Per-query filters — no skip, and the K loop is untouched: the lane reads its query's bit only for a score that has passed
//    the threshold (a few rows in a thousand).  A launch of a host-side split gets the filter of ITS first query.
// The error bound (Int4Row::eps, k_int4_nominate.hip, "GEMM sum"): that term allows a start at (t - |x^|^2) / 2 (at most 1.501 B),
// dim products (S = sum |products| <= 0.51 B) and the key's fma, (dim + 16) roundings of at most u (|s| + S) each whatever their
// order, the score twice that: 4.03 (dim + 16) u B.  This tile starts at ZERO: its dim roundings are of partial sums of at most S
// (0.51 dim u B, in the score 1.02 dim u B), and the key's fma rounds a value of at most |x^|^2 + 2 S <= 2.02 B once (2.02 u B):
// (1.02 dim + 2.02) u B, inside the term as it stands — eps is unchanged.  Non-finite values: a NaN score is never below a
// threshold and is not appended; the proof fails on its margin as for the big tile.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "vg_device.hpp"
#include "vg_flat_gemm.hpp"

namespace vg {

constexpr int kI4sThreads = 256, kI4sBN = 256;
constexpr size_t kI4sLdsMax = 160 * 1024;  // a CU's LDS (gfx950)
// the 32-dimension slots a row of row_bytes (a multiple of 16) takes in LDS: four per whole superstep, (rest + 1) / 2 of the last
__host__ __device__ constexpr int int4_small_slots(int row_bytes) { return (row_bytes >> 7) * 4 + ((((row_bytes >> 4) & 7) + 1) >> 1); }
// the kernel's dynamic LDS for rb blocks of 32 queries: the image (8 granules a slot and query) and the thresholds
__host__ __device__ constexpr size_t int4_small_lds_bytes(int rb, int row_bytes)
{
    return static_cast<size_t>(int4_small_slots(row_bytes)) * 8 * 16 * (rb * 32) + sizeof(float) * (rb * 32);
}

// The batch filter read ahead by one wave of flat_gemm_int4_small_kernel<RB, true, true> (see the header): the wave's tiles by
// ordinal i (tile first + i G, i < mine), the filter's bytes of 8 of them a window.  Only that variant has one; the others hold
// an I4sNoFilter.
struct I4sNoFilter {};
struct I4sFilterWindows {
    const uint8_t *mask;
    int64_t mask_bytes;
    int first, G, wave, lane, mine;
    uint32_t win, win_next;  // this lane's byte of window win_at, and of the one behind it
    uint64_t win_live;       // bit l: lane l's byte of `win` is not zero
    int win_at;
    __device__ __forceinline__ uint32_t load_window(int w) const
    {
        const int64_t tt = static_cast<int64_t>(first) + static_cast<int64_t>(8 * w + (lane >> 3)) * G;
        const int64_t at = tt * (kI4sBN / 8) + wave * 8 + (lane & 7);    // (a tile past the last one: past the filter's end as well)
        const uint32_t b = mask[at < mask_bytes ? at : mask_bytes - 1];  // (unconditional, like the row loads)
        return at < mask_bytes ? b : 0u;
    }
    // the first ordinal >= i (in window win_at or behind it) whose tile keeps a row; `mine`: none
    __device__ __forceinline__ int next_live(int i)
    {
        for (;;) {
            if (i >= mine) return mine;
            if ((i >> 3) != win_at) {  // (always the next window: ordinals only grow)
                win = win_next;
                win_at = i >> 3;
                win_next = load_window(win_at + 1);
                win_live = __ballot(win != 0u);
            }
            const uint64_t m = win_live & (~uint64_t(0) << (8 * (i & 7)));
            if (m != 0) return win_at * 8 + (__builtin_ctzll(m) >> 3);
            i = (win_at + 1) * 8;
        }
    }
    // windows 0 and 1 loaded; the wave's first live ordinal
    __device__ __forceinline__ int init(const uint8_t *mask_, int64_t n, int ntiles, int G_, int wave_, int lane_)
    {
        mask = mask_, mask_bytes = (n + 7) >> 3, first = static_cast<int>(blockIdx.x), G = G_, wave = wave_, lane = lane_;
        mine = (ntiles - first + G - 1) / G;
        win = load_window(0), win_next = load_window(1), win_live = __ballot(win != 0u), win_at = 0;
        return next_live(0);
    }
};

// queries: nq x dim_pad bfloat16 (gemm_operands' image, the tail from dim on zeros), nq <= 32 RB; codes: n rows of row_bytes =
// dim / 2 (dim % 32 == 0), 16-byte aligned; counts: counts[q * count_stride]; cand: cap keys a query; MASKED: mask, a bit per row,
// (n + 7) / 8 bytes at any alignment — BATCH: one for all queries, otherwise query q's at mask + q * mask_stride
template <int RB, bool MASKED = false, bool BATCH = false>
__global__ __launch_bounds__(kI4sThreads) void flat_gemm_int4_small_kernel(
    const uint16_t *__restrict__ queries, int nq, int dim_pad, const uint8_t *__restrict__ codes, int64_t n, int row_bytes,
    const float *__restrict__ norms, const float *__restrict__ thr, int thr_stride, int thr_off, int *__restrict__ counts, int count_stride,
    uint64_t *__restrict__ cand, int cap, const uint8_t *__restrict__ mask, int64_t mask_stride)
{
    static_assert(RB >= 1 && RB <= 4, "one to four blocks of 32 queries");
    static_assert(MASKED || !BATCH, "a batch filter is a filter");
    constexpr bool SKIP = MASKED && BATCH;
    constexpr int QB = RB * 32;
    extern __shared__ float gemm_lds[];
    const int ntiles = static_cast<int>((n + kI4sBN - 1) / kI4sBN), G = static_cast<int>(gridDim.x);
    if (static_cast<int>(blockIdx.x) >= ntiles) return;  // (the whole workgroup: nothing below is reached by a part of it)
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int units = row_bytes >> 4, full = units >> 3, rest = units & 7;  // 16-byte units; whole supersteps; units of the partial one
    const int a_last = (rest + 1) >> 1, nsuper = full + (rest ? 1 : 0), slots = full * 4 + a_last;
    uint4 *const img = reinterpret_cast<uint4 *>(gemm_lds);
    float *const lds_thr = gemm_lds + slots * 8 * QB * 4;

    // the image, once: granule g = ((slot 4 + m) 2 + hh) QB + q <- dimensions 32 unit + 8 m .. of query q, unit = 8 S + hh a + i
    for (int g = tid; g < slots * 8 * QB; g += kI4sThreads) {
        const int q = g % QB, x = g / QB, hh = x & 1, m = (x >> 1) & 3, slot = x >> 3, S = slot >> 2, i = slot & 3;
        const int u = hh * (S < full ? 4 : a_last) + i;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (q < nq && u < (S < full ? 8 : rest))
            v = *reinterpret_cast<const uint4 *>(queries + static_cast<int64_t>(q) * dim_pad + (8 * S + u) * 32 + 8 * m);
        img[g] = v;
    }
    if (tid < QB) lds_thr[tid] = tid < nq ? thr[static_cast<int64_t>(tid) * thr_stride + thr_off] : -INFINITY;
    __syncthreads();

    // superstep S of row tile t: this lane's 4 x 16 bytes of each of its two rows (rows past n: the last row; loads that are not
    // multiplied, or lie past the row: unit 0 of the superstep)
    auto load_step = [&](int t, int S, uint4 (&dst)[2][4]) {
        const int a = S < full ? 4 : a_last, lim = S < full ? 8 : rest;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            int64_t row = static_cast<int64_t>(t) * kI4sBN + wave * 64 + j * 32 + r;
            row = row < n ? row : n - 1;
            const uint8_t *p = codes + row * row_bytes + S * 128;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int u = h * a + i;
                dst[j][i] = *reinterpret_cast<const uint4 *>(p + ((i < a && u < lim) ? u : 0) * 16);
            }
        }
    };
    auto word = [](const uint4 &v, int m) { return m == 0 ? v.x : m == 1 ? v.y : m == 2 ? v.z : v.w; };

    // SKIP: the wave's tiles by ordinal i (tile blockIdx.x + i G) and the filter's windows over them; otherwise an empty struct
    std::conditional_t<SKIP, I4sFilterWindows, I4sNoFilter> fw;
    int ord = 0;
    if constexpr (SKIP) {
        ord = fw.init(mask, n, ntiles, G, wave, lane);
        if (ord >= fw.mine) return;  // (the wave alone: there is no barrier behind the image's)
    }

    f32x16 acc[RB][2];
    uint4 cur[2][4], nxt[2][4];
    int t = static_cast<int>(blockIdx.x) + ord * G;
    load_step(t, 0, cur);
    while (t < ntiles) {
        // the tile this wave computes next (ntiles or more: none).  SKIP: this tile's filter bits leave the window first — lane
        // (r, h)'s rows 32 j + r are bit r & 7 of the byte that lane 8 (ord & 7) + 4 j + (r >> 3) holds
        int t_next = t + G;
        bool kept[2] = {true, true};
        if constexpr (SKIP) {
#pragma unroll
            for (int j = 0; j < 2; j++) kept[j] = (__shfl(fw.win, 8 * (ord & 7) + 4 * j + (r >> 3)) >> (r & 7)) & 1u;
            ord = fw.next_live(ord + 1);
            t_next = static_cast<int>(blockIdx.x) + ord * G;  // (ord <= mine: at most ntiles - 1 + G)
        }
        const int64_t n0 = static_cast<int64_t>(t) * kI4sBN + wave * 64;
        float xn[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int64_t nn = n0 + j * 32 + r;
            xn[j] = norms[nn < n ? nn : n - 1];
        }
#pragma unroll
        for (int b = 0; b < RB; b++)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[b][j][e] = 0.0f;
        for (int S = 0; S < nsuper; S++) {
            // the next superstep's loads — of the next tile behind the last one; past the stream's end: the last tile's first again,
            // never multiplied (unconditional: a load under a condition makes the compiler drain the queue)
            const bool last = S + 1 == nsuper;
            const int tn = last ? (t_next < ntiles ? t_next : ntiles - 1) : t;
            load_step(tn, last ? 0 : S + 1, nxt);
            const int a = S < full ? 4 : a_last, lim = S < full ? 8 : rest;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (i >= a) break;  // (wave-uniform)
                const bool past = h * a + i >= lim;  // lane half 1's unit behind an odd `rest`
                const uint4 *pa = img + ((S * 4 + i) * 4 * 2 + h) * QB + r;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    uint4 fa[RB], fb[2];
#pragma unroll
                    for (int b = 0; b < RB; b++) fa[b] = pa[m * 2 * QB + b * 32];
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        fb[j] = int4_word_bf16(word(cur[j][i], m) ^ 0x88888888u);
                        if (past) fb[j] = make_uint4(0u, 0u, 0u, 0u);
                    }
#pragma unroll
                    for (int b = 0; b < RB; b++)
#pragma unroll
                        for (int j = 0; j < 2; j++)
                            acc[b][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(vg_bf16x8, fa[b]),
                                                                               __builtin_bit_cast(vg_bf16x8, fb[j]), acc[b][j], 0, 0, 0);
                    // (a slice at a time: left to itself the scheduler hoists every slice's reads and conversions of the superstep
                    // and takes a register for each)
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int i = 0; i < 4; i++) cur[j][i] = nxt[j][i];
        }
        // the appends (gemm_epilogue's MODE 2): C/D map of the 32 x 32 instruction — column = lane & 31 (the row of the block),
        // register e = query (e & 3) + 8 (e >> 2) + 4 h of the block
        bool parked = false;
        int park_pos = 0, park_q = 0;
        uint64_t park_key = 0;
        auto store_parked = [&]() {
            if (park_pos < cap) cand[static_cast<int64_t>(park_q) * cap + park_pos] = park_key;
        };
        // (what depends only on the lane is derived from this INSIDE the tile loop: left to itself the compiler tests the lane's
        // 16 RB query indices against nq once, ahead of the loop, and keeps the lane masks in scalar registers it has to spill)
        int hv = 4 * h;
        asm volatile("" : "+v"(hv));
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int64_t nn = n0 + j * 32 + r;
            const bool row_ok = nn < n && kept[j];
#pragma unroll
            for (int b = 0; b < RB; b++) {
                // a block's 16 scores and compares with no branch between them; only a block in which something passed looks again
                float sc[16], tq[16];
                bool any = false;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const float4 tv = *reinterpret_cast<const float4 *>(lds_thr + b * 32 + 8 * g + 4 * h);
                    tq[4 * g] = tv.x, tq[4 * g + 1] = tv.y, tq[4 * g + 2] = tv.z, tq[4 * g + 3] = tv.w;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        sc[4 * g + e] = __builtin_fmaf(-2.0f, acc[b][j][4 * g + e], xn[j]);
                        any |= sc[4 * g + e] < tq[4 * g + e];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);  // (block by block: hoisted, the 32 RB scores of a row block are all live at once)
                if (any && row_ok) {
#pragma unroll
                    for (int e = 0; e < 16; e++) {
                        const int q = b * 32 + (e & 3) + 8 * (e >> 2) + hv;
                        asm volatile("" : "+v"(sc[e]));  // (compared again here: 16 lane masks kept per block spill the scalar registers)
                        if (!(sc[e] < tq[e]) || q >= nq) continue;
                        if constexpr (MASKED && !BATCH)  // (only now: for the few scores that passed)
                            if (!mask_bit(mask + static_cast<int64_t>(q) * mask_stride, nn)) continue;
                        if (parked) store_parked();
                        park_pos = atomicAdd(&counts[static_cast<int64_t>(q) * count_stride], 1);
                        park_q = q;
                        park_key = make_key(sc[e], static_cast<uint32_t>(nn), false);
                        parked = true;
                    }
                }
            }
        }
        if (parked) store_parked();
        t = t_next;
    }
}

}  // namespace vg
