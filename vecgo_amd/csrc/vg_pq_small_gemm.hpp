// vg_pq_small_gemm.hpp — the PQ nomination's append GEMM (from the codes) for ONE query tile of up to 128 queries
// (flat_gemm_pq_small_kernel): bf16 queries against rows that exist only as PQ codes, scoring in flat_gemm_codes_big_kernel's space,
//     s = |x^|^2 - 2 q.x^,   q and the decoded row x^ both rounded to bfloat16 — the operands the image mode and the big
// code-gathered tile multiply, bit for bit: the row operand is an entry of the decoded codebook (NomImage::rows of a from_codes
// state, [dim_pad / 8][256] entries of 16 bytes, pq_codebook_bf16_kernel), the query operand gemm_operands' image.
// Kept in a header so that tools/ubench can time the same code; launched by k_pq_small.hip.  L2, MODE 2 (append); row filters: the last point below.
//
// The counterpart of vg_int4_small_gemm.hpp and vg_sq8_small_gemm.hpp — a single query tile, so a row is consumed by exactly one
// wave, LDS holding the queries' image alone — with one difference that shapes it: there is nothing to convert.  With 8 dimensions
// per sub-quantizer a decoded centroid in bfloat16 is 16 bytes, exactly one lane's operand of v_mfma_f32_32x32x16_bf16 (row
// lane & 31, k-slice lane >> 5, 8 values): a lane GATHERS its operand by its row's code byte from the codebook into the register
// the matrix instruction reads.  No LDS, no vector ALU between the load and the multiply; what the vector ALU does is the address.
//  * 256 threads as 1 x 4 waves; a row tile is 256 rows, wave w owns rows 64 w .. 64 w + 63 of it as two 32-row blocks; workgroups
//    are persistent over the row tiles (t = blockIdx.x, + gridDim.x, ...).  A row past n re-reads the last row's codes (never
//    appended).
//  * K is walked in STEPS of 16 dimensions = two sub-quantizers, one matrix instruction per (query block, row block).  In step i
//    lane (r, h) of row block j needs entry (2 i + h, codes[row][2 i + h]): one 16-byte load from the 4 KB slice 2 i + h of the
//    codebook (L2-resident: 393 KB at m = 96; two slices a step and wave, 8 KB a step through a CU's vector cache).  The slice is
//    wave-uniform up to h, so the load is the scalar-base form: base = slice 2 i, offset = (h 256 + code) 16 — three vector
//    instructions a gather (shift, and-or with h 256, shift by 4), read from the ISA.
//  * padding: for sub-quantizers j >= m up to dim_pad / 8 the codebook holds zeros for EVERY code and the query image zeros, so an
//    odd m needs no mask — lane half 1 of the last step gathers entry (m, whatever byte follows the row) = zeros.  dim_pad is a
//    multiple of 64, so slices 0 .. 2 steps - 1 all exist (2 steps <= m + 1 <= dim_pad / 8) and every index (slice, byte) is
//    inside [dim_pad / 8][256] whatever the byte.
//  * the code bytes: rows are row-major, m bytes each, at ANY alignment (m is not a multiple of anything).  A CHUNK is 8 steps =
//    16 sub-quantizers = 16 code bytes of a row: a lane reads its two rows' 16 bytes of a chunk with one 16-byte load each, at
//    whatever alignment they have (the target's unaligned access mode: global_load_dwordx4 at byte alignment, the memory system
//    splits it where it crosses a line — the widest load the hardware allows, whatever m).  Step p of the chunk uses byte 2 p + h:
//    word p >> 1, bit 16 (p & 1) + 8 h, one v_bfe_u32.  The only read that could leave the n m bytes of the codes is one of the
//    last 15 bytes' rows: its address is clamped to n m - 16 and the loaded 16 bytes shifted right by the same number of bytes
//    (pq_small_shr_bytes; zeros come in — positions >= m, which meet zero slices or steps that are not multiplied).  n m >= 16 is
//    the launch's condition.
//  * the dependent chain code -> address -> gather is never waited for inside a chunk: the stream of (tile, chunk) positions
//    u = 0, 1, ... of a workgroup runs three stages deep.  During chunk u the matrix instructions consume the ring (the gathers of
//    u, issued during u - 1), the gathers of u + 1 are issued from the codes of u + 1 (loaded during u - 1), and the codes of
//    u + 2 are loaded first thing.  Retirement is in order and the code load of u + 2 is issued BEHIND the gathers of u and ahead of
//    those of u + 1, so the wait for it at the start of chunk u + 1 is a counted one that leaves the 16 gathers issued after it in
//    flight.  (The issue's sketch read a whole tile's codes ahead; two chunks ahead is the same guarantee at 16 registers for any
//    m — a tile's codes are 80 registers a lane at m = 318.)  Across a tile's end the stream goes on into the next tile: its first
//    chunk's codes and gathers fly under the tile before it.  Past the stream's end it repeats the last tile's first chunk.
//  * gathers in flight: a ring of kPqsDepth = 8 steps x 2 row blocks x 16 bytes = 64 VGPRs.  Slot p is refilled unconditionally as
//    soon as step p's matrix instructions have been issued (they read the slot; the load behind them overwrites it when it lands —
//    there is no conversion that could free the slot earlier).  Steps past the row's last (the last chunk of an m that is no
//    multiple of 16) gather from the last step's slices and are not multiplied.  What the compiler made of it (read from the
//    ISA): the slots are reused in place — the load that refills v[84:87] follows the matrix instruction that read v[84:87], no copy
//    at a chunk's end as in both siblings — and every wait in the K loop is counted: vmcnt(17) and vmcnt(16) before a step's two
//    matrix instructions, vmcnt(17) / (16) for the codes at a chunk's start.  The tile's end: the epilogue's first wait is
//    vmcnt(19), for the tile's two norms — loaded ahead of the tile's first chunk, so older than all in flight — and the next
//    position's 16 gathers and 2 code loads fly under the epilogue.  (The chunk loop is a do-while for that: nchunks >= 1 always,
//    but with a path around the loop the compiler took the norms for the youngest loads and waited vmcnt(1) there, a drain at every
//    tile's end and for m <= 16 at every chunk.)  Where the ring DOES drain: at an append — the returning atomic is waited for
//    with vmcnt(0), inside the branch that only a lane with a row below its threshold takes; and a tile's first steps wait two
//    loads deeper than the ring asks, because the norms' two loads lie between two chunks' gathers (loading them inside the chunk
//    loop, to make every chunk alike, was tried: the compiler hoists them back out, or, the address hidden from it, sinks them
//    behind the loop and drains there).  Gathers run one chunk (128 dimensions) ahead, codes two.  This needs the VGPR form of the
//    matrix instruction (the unit's flag in the Makefile): with accumulators in AGPRs the compiler copied all 32 RB of them to VGPRs
//    and back around every step.  Registers, LDS, occupancy per RB: profiles/kernel_resources.txt (146 / 190 / 222 / 254 VGPRs, no
//    AGPRs, no scratch, 3 / 2 / 2 / 2 waves a SIMD).
//  * the image is RESIDENT in LDS for the whole kernel (the reasons are the INT4 tile's: a streamed piece would wait behind every
//    gather in flight): the K loop has no barrier and no LDS write.  Layout: granule (i 2 + h) QB + q, 16 bytes each, QB = 32 RB:
//    dimensions 16 i + 8 h .. + 8 of query q in natural order — no k-permutation, the row operand's order is the dimension order.
//    32 ceil(m / 2) QB + 4 QB bytes with the thresholds (pq_small_lds_bytes <= 160 KiB): RB = 4 fits up to m = 78, RB = 3 up to
//    106, RB = 2 up to 158, one block up to m = 318 (dim 2544).  What does not fit is split ON THE HOST into the fewest launches
//    of equally many blocks (launch_pq_small_gemm, k_pq_small.hip: 97 .. 128 queries at m = 96 run as two launches of two blocks);
//    above m = 318 the batch keeps the scan (pq_small_tile_fits).
//    An operand read (fixed i and 32-query block) is 32 consecutive granules per lane half.  ds_read_b128 serves 16 lanes a pass;
//    the 16 lanes of a pass read 16 consecutive granules = 256 contiguous bytes = each of the 64 banks once: no conflict, whatever
//    QB (the two lane halves are in different passes).  Each read feeds the wave's two row blocks: 2 RB matrix instructions for RB
//    ds_read_b128 per step.
//  * the epilogue is gemm_epilogue's append (vg_flat_gemm.hpp) as in both siblings: score = fma(-2, acc, |x^|^2), compared with
//    the query's threshold (in LDS; -Inf for the padded queries of the last block: they never append), a returning atomic on the
//    query's counter parked until the tile's end, the key make_key(score, row).
//  * row filters (vg_index_enable_pq_nomination_from_codes' on & 4) are variants of their own, MASKED and BATCH template parameters:
//    the unfiltered instantiations are the code they were (the same instructions but for one kernel-argument offset, the same
//    registers: diffed against the ISA of the kernel without the parameters).
//    Per-query filters (MASKED, not BATCH) — the K loop is untouched: a lane reads its query's bit only for a score that has passed
//    the threshold, inside the branch that drains for the append's atomic anyway.  A launch of a host-side split gets the filter
//    of ITS first query.
//    BATCH — one filter for all queries.  A wave's 64 rows of a tile are 8 bytes of it; a slice whose 8 bytes are zero is never
//    WALKED: no code load, no gather, no matrix instruction, no epilogue — and the gathers are what a pass costs.  After the image's
//    barrier the four waves of a workgroup have nothing in common (no barrier, no LDS write), so each wave walks its OWN stream of
//    (tile, chunk) positions over the tiles whose slice keeps a row; a wave without one leaves behind that barrier.  advance()
//    runs two chunks ahead of the matrix instructions and must know the next such tile without waiting for a load, so the filter
//    is held as a wave-uniform BITMAP of a WINDOW of the wave's tiles (SliceFilterWindows, vg_slice_windows.hpp): one vector load, lane l the 8 bytes of
//    the wave's slice in tile (64 w + l) of the workgroup's sequence (at any alignment; a slice that sticks out of the filter —
//    the last tile's — reads the filter's last 8 bytes and shifts; the launch takes this variant from n = 64 up), a ballot of
//    "not zero", and s_ff1_i32_b64 from the current position steps to the next tile: scalar work between two chunks.
//    The window is 64 tiles, a lane each — one load instruction whatever the length, so the longest one a ballot holds: with
//    G workgroups it covers 64 G tiles, which is every tile a wave ever has up to 12.6M rows at 768 workgroups: ONE filter load a wave
//    and kernel, in the prologue.  Where a wave has more, the next window is loaded WHEN THE CURRENT ONE IS SPENT and waited for
//    there, a drain of the ring once in 64 of the wave's tiles (384 chunks at m = 96, walked or not).  Loading it a window ahead,
//    as flat_gemm_int4_small_kernel does with its windows of 8, was built first and read in the ISA: the load sits in the rare
//    branch of advance(), the compiler lands it in a temporary and copies it to the window's register behind the branch's merge,
//    with s_waitcnt vmcnt(0) in front of the copy — on EVERY way through the merge, i.e. a drain at every tile's end, what the
//    do-while above exists to avoid.  As built: the ways through advance() that stay inside a window have no vector-memory
//    operation and no wait; the K loop's waits are vmcnt(17) / vmcnt(16) as unfiltered; vmcnt(0) stands behind the window's load
//    alone (and at the appends).  Past its end the stream repeats the first chunk of the tile it is on — the last one it walked,
//    in range — never a skipped slot.  A walked slice's rows still test their own bit: the two filter bytes with a lane's rows'
//    bits are loaded beside the tile's norms (the epilogue's first wait is vmcnt(19) as before: both are older than everything
//    in flight) and stand beside `row < n`; bits at or past n can make the last slice walked, never a row appended.
//    Registers (profiles/kernel_resources.txt): 150 / 192 / 226 / 256 VGPRs BATCH, 150 / 192 / 224 / 256 per query, no AGPRs, no
//    scratch, the unfiltered occupancy.  Measured: the comment above kPqNomCodesMaskedMinPairs (k_pq_nominate.hip).
// The error bound (pq_nominate_eps, k_pq_nominate.hip).  The operands are the image's bit for bit, so the bfloat16 term
// (2^-7 + 2^-16)(|q|^2 + |x^|^2) is the image mode's; what differs is the sum's order and start.  The formula allows 4 dim u
// (|q|^2 + |x^|^2), u = 2^-24, for "the GEMM's fp32 accumulation and the norm's".  This tile starts at ZERO and adds dim products
// in the matrix unit, S = sum |products| <= (1 + 2^-8)^2 |q||x^| <= 0.51 (|q|^2 + |x^|^2): every partial sum is at most S, dim
// roundings of at most u S each whatever their order: 0.51 dim u (|q|^2 + |x^|^2) in the sum, 1.02 dim u in the score (twice the
// sum).  The key's fma rounds |x^|^2 - 2 acc once, a value of at most |x^|^2 + 2 S <= 2.02 (|q|^2 + |x^|^2): 2.02 u.  The norm
// (pq_norms_kernel: dim fmas and a 6-step tree over lanes, non-negative terms) is off by at most (dim + 6) u |x^|^2 (1 + ...),
// 1.01 (dim + 6) u.  Together (2.03 dim + 8.1) u (|q|^2 + |x^|^2) <= 4 dim u for every dim >= 8 (m >= 1): inside the formula —
// which already covers the zero-started 32-row bf16 tile the image mode runs for these batch sizes — so eps is unchanged.
// Non-finite values: a NaN score is never below a threshold and is not appended; the proof fails on its margin as for the big tile.
//
// Measured (MI355X, m = 96, the GEMM's profile scope; before the tile's end stopped draining — a run after it: within 3 %): one pass over 1M
// rows 0.184 ms at 8 queries, 0.189 at 32, 0.200 at 64, 0.220 at 96, two passes 0.388 at 128; 10M rows 1.73 .. 1.81 ms a pass.  The
// limiter is not established: HBM (96 MB of codes a pass) and the matrix unit are both under a tenth of the time; the 1.5 GB of
// 16-byte codebook entries a pass go through the vector caches at 8.3 .. 8.7 TB/s, 13.5 .. 14.2 B a clock and CU, 21 .. 22 % of
// their nominal 64 B a clock — too far below it to call the gather's throughput the bound; latency or occupancy may be.  The
// whole table and the crossover: the comment above kPqNomCodesSmallMinPairs (k_pq_nominate.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "vg_device.hpp"
#include "vg_flat_gemm.hpp"
#include "vg_slice_windows.hpp"

namespace vg {

constexpr int kPqsThreads = 256, kPqsBN = 256, kPqsDepth = 8;
constexpr size_t kPqsLdsMax = 160 * 1024;  // a CU's LDS (gfx950)
// the 16-dimension steps of a row of m sub-quantizers
__host__ __device__ constexpr int pq_small_steps(int m) { return (m + 1) >> 1; }
// the kernel's dynamic LDS for rb blocks of 32 queries: the image (two granules a step and query) and the thresholds
__host__ __device__ constexpr size_t pq_small_lds_bytes(int rb, int m)
{
    return static_cast<size_t>(pq_small_steps(m)) * 2 * 16 * (rb * 32) + sizeof(float) * (rb * 32);
}

// 16 bytes shifted right by s bytes (0 .. 15), zeros coming in at the top
__device__ __forceinline__ uint4 pq_small_shr_bytes(uint4 v, uint32_t s)
{
    const uint32_t bs = s & 3u;
    uint32_t a0 = __builtin_amdgcn_alignbyte(v.y, v.x, bs), a1 = __builtin_amdgcn_alignbyte(v.z, v.y, bs),
             a2 = __builtin_amdgcn_alignbyte(v.w, v.z, bs), a3 = __builtin_amdgcn_alignbyte(0u, v.w, bs);
    if (s & 4u) a0 = a1, a1 = a2, a2 = a3, a3 = 0u;
    if (s & 8u) a0 = a2, a1 = a3, a2 = 0u, a3 = 0u;
    return make_uint4(a0, a1, a2, a3);
}

static_assert(kPqsBN == kSliceBN, "the filter windows' row tile is this tile's");

// queries: nq x dim_pad bfloat16 (gemm_operands' image, the tail from dim on zeros), nq <= 32 RB, dim_pad >= 16 steps; codes: n rows
// of m bytes, n m >= 16; cb16: the decoded codebook, at least 2 steps slices of 256 entries; counts: counts[q * count_stride];
// cand: cap keys a query; MASKED: mask, a bit per row, (n + 7) / 8 bytes at any alignment — BATCH: one for all queries (n >= 64: 8
// bytes of it exist), otherwise query q's at mask + q * mask_stride (a stride of 0: one for all, without the skip)
template <int RB, bool MASKED = false, bool BATCH = false>
__global__ __launch_bounds__(kPqsThreads) void flat_gemm_pq_small_kernel(
    const uint16_t *__restrict__ queries, int nq, int dim_pad, const uint8_t *__restrict__ codes, int64_t n, int m,
    const uint4 *__restrict__ cb16, const float *__restrict__ norms, const float *__restrict__ thr, int thr_stride, int thr_off,
    int *__restrict__ counts, int count_stride, uint64_t *__restrict__ cand, int cap, const uint8_t *__restrict__ mask, int64_t mask_stride)
{
    static_assert(RB >= 1 && RB <= 4, "one to four blocks of 32 queries");
    static_assert(MASKED || !BATCH, "a batch filter is a filter");
    constexpr bool SKIP = MASKED && BATCH;
    constexpr int QB = RB * 32, D = kPqsDepth;
    extern __shared__ float gemm_lds[];
    const int ntiles = static_cast<int>((n + kPqsBN - 1) / kPqsBN), G = static_cast<int>(gridDim.x);
    if (static_cast<int>(blockIdx.x) >= ntiles) return;  // (the whole workgroup: nothing below is reached by a part of it)
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nsteps = pq_small_steps(m), nchunks = (nsteps + D - 1) / D;
    const int64_t total = n * m;  // the bytes of the codes
    uint4 *const img = reinterpret_cast<uint4 *>(gemm_lds);
    float *const lds_thr = gemm_lds + nsteps * 2 * QB * 4;

    // the image, once: granule g = (i 2 + hh) QB + q <- dimensions 16 i + 8 hh .. + 8 of query q (< dim_pad)
    for (int g = tid; g < nsteps * 2 * QB; g += kPqsThreads) {
        const int q = g % QB, x = g / QB;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (q < nq) v = *reinterpret_cast<const uint4 *>(queries + static_cast<int64_t>(q) * dim_pad + 8 * x);
        img[g] = v;
    }
    if (tid < QB) lds_thr[tid] = tid < nq ? thr[static_cast<int64_t>(tid) * thr_stride + thr_off] : -INFINITY;
    __syncthreads();

    // where the 16 code bytes of chunk c of this lane's row in block j of tile t start, and how far that is past the last place
    // from which 16 bytes can be read (0 for all but the rows inside the last 15 bytes)
    auto code_at = [&](int t, int c, int j, uint32_t &over) {
        const int64_t row = static_cast<int64_t>(t) * kPqsBN + wave * 64 + j * 32 + r;
        const int64_t a = (row < n ? row : n - 1) * m + 16 * c, last = total - 16;
        over = a > last ? static_cast<uint32_t>(a - last) : 0u;  // (< 16: a < total)
        return a > last ? last : a;
    };
    auto load_codes = [&](int t, int c, uint4 (&dst)[2]) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            uint32_t over;
            __builtin_memcpy(&dst[j], codes + code_at(t, c, j, over), 16);  // (any alignment)
        }
    };
    // the loaded bytes as the chunk's: shifted where the address was clamped
    auto take_codes = [&](int t, int c, const uint4 (&src)[2], uint4 (&dst)[2]) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            uint32_t over;
            (void)code_at(t, c, j, over);
            dst[j] = pq_small_shr_bytes(src[j], over);
        }
    };
    // step p of chunk c, both row blocks, from the chunk's code bytes (steps past the last: the last step's slices, any byte)
    const uint32_t bit_h = 8u * static_cast<uint32_t>(h), ent_h = 256u * static_cast<uint32_t>(h);
    auto gather = [&](int c, int p, const uint4 (&cd)[2], uint4 (&dst)[2]) {
        const int i = c * D + p, ii = i < nsteps ? i : nsteps - 1;
        const uint4 *slice = cb16 + static_cast<int64_t>(ii) * 512;  // (wave-uniform)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t w = (p >> 1) == 0 ? cd[j].x : (p >> 1) == 1 ? cd[j].y : (p >> 1) == 2 ? cd[j].z : cd[j].w;
            const uint32_t code = (w >> (16u * (p & 1) + bit_h)) & 0xFFu;
            dst[j] = slice[ent_h + code];
        }
    };
    // SKIP: the wave's tiles by ordinal (tile blockIdx.x + ordinal G) and the filter's windows over them; otherwise an empty struct.
    // ord1: the ordinal of the tile the stream is on — fw.mine: the stream has ended
    std::conditional_t<SKIP, SliceFilterWindows, SliceNoFilter> fw;
    int ord1 = 0;
    if constexpr (SKIP) {
        ord1 = fw.init(mask, n, ntiles, G, wave, lane);
        if (ord1 >= fw.mine) return;  // (the wave alone: there is no barrier behind the image's)
    }
    // the stream's next position behind (t, c): the next chunk, the next tile's first, past the end the last tile's first again
    // (SKIP: the wave's next tile whose slice keeps a row; past the end the tile it is on — a walked one, in range — again)
    auto advance = [&](int &t, int &c) {
        if (c + 1 < nchunks) {
            c++;
        } else {
            c = 0;
            if constexpr (SKIP) {
                ord1 = fw.next_live(ord1 + 1);
                if (ord1 < fw.mine) t = static_cast<int>(blockIdx.x) + ord1 * G;
            } else {
                t = t + G < ntiles ? t + G : ntiles - 1;
            }
        }
    };

    f32x16 acc[RB][2];
    uint4 ring[D][2], cur[2], nxt[2];
    // the stream's start: the codes of position 0 and its gathers, the codes of position 1
    int t1 = static_cast<int>(blockIdx.x), c1 = 0;  // the position whose gathers are issued next
    if constexpr (SKIP) t1 += ord1 * G;
    const int c0 = c1;
    int t = t1, ord = ord1;  // the tile that is computed, SKIP: and its ordinal
    load_codes(t1, c1, nxt);
    take_codes(t1, c1, nxt, cur);
    advance(t1, c1);
    __builtin_amdgcn_sched_barrier(0);
    load_codes(t1, c1, nxt);  // (ahead of the gathers, as in the loop: the same count of loads lies behind it on both ways in)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < D; p++) {
        gather(c0, p, cur, ring[p]);
        __builtin_amdgcn_sched_barrier(0);  // (in the ring's order: the K loop waits for its slots by count)
    }
    auto more = [&]() {
        if constexpr (SKIP)
            return ord < fw.mine;
        else
            return t < ntiles;
    };
    while (more()) {
        const int64_t n0 = static_cast<int64_t>(t) * kPqsBN + wave * 64;
        // the tile's norms: two loads ahead of the tile's first chunk (its first steps wait two loads deeper than the ring asks), and
        // older than everything in flight when the epilogue reads them
        float xn[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int64_t nn = n0 + j * 32 + r;
            xn[j] = norms[nn < n ? nn : n - 1];
        }
        // SKIP: the filter's bytes with the rows' bits, beside the norms and as old as they are when the epilogue reads them
        uint32_t fbyte[2] = {0xFFu, 0xFFu};
        if constexpr (SKIP) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int64_t nn = n0 + j * 32 + r;
                fbyte[j] = mask[(nn < n ? nn : n - 1) >> 3];
            }
        }
        int t_next = t + G, ord_next = 0;  // SKIP: the position behind the tile's last chunk
#pragma unroll
        for (int b = 0; b < RB; b++)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[b][j][e] = 0.0f;
        int c = 0;
        do {  // (nchunks >= 1: a loop the compiler knows to run — a path around it would set the waits behind it)
            // (t1, c1) is the position behind (t, c): its codes have been in flight for a chunk; the position behind it is loaded now
            take_codes(t1, c1, nxt, cur);
            const int cg = c1;
            if constexpr (SKIP) t_next = t1, ord_next = ord1;
            advance(t1, c1);
            __builtin_amdgcn_sched_barrier(0);
            load_codes(t1, c1, nxt);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < D; p++) {
                const int i = c * D + p;
                if (i < nsteps) {  // (wave-uniform; no vector-memory operation inside)
                    const uint4 *pa = img + (i * 2 + h) * QB + r;
                    uint4 fa[RB];
#pragma unroll
                    for (int b = 0; b < RB; b++) fa[b] = pa[b * 32];
#pragma unroll
                    for (int b = 0; b < RB; b++)
#pragma unroll
                        for (int j = 0; j < 2; j++)
                            acc[b][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(vg_bf16x8, fa[b]),
                                                                               __builtin_bit_cast(vg_bf16x8, ring[p][j]), acc[b][j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                gather(cg, p, cur, ring[p]);  // the slot's next gather, unconditionally
                __builtin_amdgcn_sched_barrier(0);
            }
        } while (++c < nchunks);
        // the appends (gemm_epilogue's MODE 2): C/D map of the 32 x 32 instruction — column = lane & 31 (the row of the block),
        // register e = query (e & 3) + 8 (e >> 2) + 4 h of the block
        bool parked = false;
        int park_pos = 0, park_q = 0;
        uint64_t park_key = 0;
        auto store_parked = [&]() {
            if (park_pos < cap) cand[static_cast<int64_t>(park_q) * cap + park_pos] = park_key;
        };
        // (what depends only on the lane is derived from this INSIDE the tile loop, as in the siblings: left to itself the compiler
        // tests the lane's 16 RB query indices against nq once, ahead of the loop, and keeps the lane masks in scalar registers)
        int hv = 4 * h;
        asm volatile("" : "+v"(hv));
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int64_t nn = n0 + j * 32 + r;
            const bool row_ok = nn < n && (!SKIP || ((fbyte[j] >> (nn & 7)) & 1u));
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
        t = t_next, ord = ord_next;
    }
}

}  // namespace vg
