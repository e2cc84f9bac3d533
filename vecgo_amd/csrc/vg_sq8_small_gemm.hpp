// vg_sq8_small_gemm.hpp — the SQ8 nomination's append GEMM (from the codes) for ONE query tile of up to 128 queries
// (flat_gemm_sq8_small_kernel): bf16 queries (scaled by the quantizer's inverse scales) against the index's SQ8 code TILES, scoring
// in flat_gemm_sq8_big_kernel's space,
//     s' = |x^|^2 - 2 (q o inv).c'   (Dot: -(q o inv).c'),   c' = code - 128 exact in bfloat16, the image of q o inv the only rounded operand.
// Kept in a header so that tools/ubench can time the same code; launched by k_sq8_small.hip.  Row filters: the last point below.
//
// The counterpart of vg_int4_small_gemm.hpp — a single query tile, so a row is consumed by exactly one wave and goes from global
// memory straight into the registers that feed v_mfma_f32_32x32x16_bf16, LDS holding the queries' image alone — but not a copy: the
// codes are not row-major rows.  They are the scan's tiles, [64-row tile][16-dimension group][row] of 16 bytes, zero past dim and
// past n (sq8_retile_kernel), and the design follows from that.
//  * 256 threads as 1 x 4 waves; a row tile is 256 rows = four 64-row code tiles, wave w owns code tile 4 t + w as two 32-row
//    blocks; workgroups are persistent over the row tiles (t = blockIdx.x, + gridDim.x, ...).  A code tile past n_tiles re-reads the
//    last one (its rows are >= n: never appended).  A code tile that exists holds all 64 rows and all 16 bytes of every group: no
//    load ever leaves the allocation.
//  * K is walked in STEPS of 32 dimensions = two groups.  The matrix instruction gives lane (r = lane & 31, h = lane >> 5) row r of
//    the block and the k-slice h: in step i lane (r, h) of row block j loads the 16-byte piece of group 2 i + h,
//        tiles[(tile groups + 2 i + h) 64 + 32 j + r],
//    so each half-wave reads 512 contiguous bytes — four whole cache lines per load instruction, nothing read twice, where the
//    row-major INT4 rows need a pair of lanes and four loads to take a line.  A piece is 16 codes: its low and high 8 bytes are the
//    two row operands m = 0, 1, and matrix instruction (i, m) multiplies, in lane half h, dimensions 32 i + 16 h + 8 m .. + 8.  The
//    query operand takes the SAME k-permutation per lane half — granule (i, m, h) of the image holds exactly those 8 dimensions — so
//    every product pairs q_d with c'_d and the sum over a row is the dot product in another order.
//  * the row operand is bf16(code - 128): code ^ 0x80 read as a signed byte is the centred value; int -> float ->
//    v_cvt_pk_bf16_f32, all exact, as the big tile's fill does it (sq8_half_bf16).
//  * an odd group count (dim % 32 in 1 .. 16): lane half 1's group of the last step does not exist.  Its lanes re-read that step's
//    group 2 i (lane half 0's: it exists) and their operand is replaced by zeros; the image's granules there are zeros too.  Codes
//    past dim inside the last group are zero bytes, -128 as operands: they meet zeros of the image.
//  * the image is RESIDENT in LDS for the whole kernel (the reasons are the INT4 tile's: a streamed piece would wait behind every
//    row load in flight, retirement being in order): the K loop has no barrier and no LDS write.  64 bytes a step and query: QB = 32 RB
//    queries a launch, RB = 1 .. 4; RB = 4 fits up to dim 608, RB = 3 up to 832, RB = 2 up to 1248 and one block up to dim 2528
//    (sq8_small_lds_bytes <= 160 KiB).  What does not fit is split ON THE HOST into the fewest launches of equally many blocks
//    (launch_sq8_small_gemm, k_sq8_small.hip: 97 .. 128 queries at dim 768 run as two launches of two blocks); where one block does
//    not fit the batch keeps the scan (sq8_small_tile_fits).
//    Layout: granule ((i 2 + m) 2 + h) QB + q, 16 bytes each.  An operand read (fixed i, m and 32-query block) is 32 consecutive
//    granules per lane half.  ds_read_b128 serves 16 lanes a pass; the 16 lanes of a pass read 16 consecutive granules = 256
//    contiguous bytes = each of the 64 banks once: no conflict, whatever QB (the two lane halves are in different passes).  Each
//    read feeds the wave's two row blocks: 4 RB matrix instructions for 2 RB ds_read_b128 per step.
//  * loads in flight: a ring of kS8sDepth = 8 steps, 16 pieces of 16 bytes a lane (64 VGPRs; 64 KiB a workgroup — what one
//    workgroup a CU needs to cover the HBM latency at its share of the bandwidth, and the widest form (RB = 4: 128 accumulators)
//    still has the registers for it under launch_bounds(256): profiles/kernel_resources.txt).  Slot p of the ring holds step
//    c 8 + p of chunk c.  When slot p has been taken into the conversion its load for the NEXT chunk — across a tile's end the next
//    tile's first chunk — is issued at once, before the step's matrix instructions and unconditionally (a load under a condition
//    makes the compiler drain the queue): the loads of a tile's first chunk fly under the tile before it.  Steps past the row's
//    last (the last chunk of a row that is no multiple of 256 dimensions) re-read the last step — the same cache lines — and are
//    not multiplied.  Inside a chunk the waits are counted (read from the ISA: vmcnt(18) per step, the 16 pieces and a tile's two
//    norms).  NOT reached: a ring that never drains.  The compiler lands a chunk's loads in fresh registers and copies them into
//    the loop's at the chunk's end, which waits for all of them — so the loads run one chunk, 256 dimensions, ahead, as the INT4
//    tile's run one superstep ahead, and the registers are the ring's twice (RB = 1: 182 VGPRs, two workgroups a CU).  Converting a
//    slot before its load is issued did not make it reuse the registers; loads in inline assembly with hand-counted waits were
//    not tried.
//  * the epilogue is gemm_epilogue's append (vg_flat_gemm.hpp) as in the INT4 small tile: score = fma(-2, acc, |x^|^2) (Dot: -acc),
//    compared with the query's threshold (in LDS; -Inf for the padded queries of the last block: they never append), a returning
//    atomic on the query's counter parked until the tile's end, the key make_key(score, row) — the form Sq8CodesRow's verify pair reads.
//  * row filters (vg_index_enable_sq8_nomination_from_codes' on & 4) are variants of their own, MASKED and BATCH template parameters:
//    the unfiltered instantiations keep their vector instructions, waits and registers (diffed against the ISA of the kernel
//    without the parameters: one s_add_i32 at the tile loop's end became an s_mov_b32 and the scalar registers are numbered
//    differently; VGPRs, AGPRs and occupancy as they were, profiles/kernel_resources.txt).
//    Per-query filters (MASKED, not BATCH) — the K loop is untouched (vmcnt(18) / (19) as unfiltered): a lane reads its query's bit
//    only for a score that has passed the threshold, inside the branch that drains for the append's atomic anyway.  A launch of a
//    host-side split gets the filter of ITS first query.
//    BATCH — one filter for all queries.  A wave's 64 rows of a row tile are exactly one code tile, groups x 1024 contiguous
//    bytes, and 8 bytes of the filter; a code tile whose 8 bytes are zero is never loaded, converted or multiplied — HBM bytes
//    not read, on the one small tile that is HBM-bound.  After the image's barrier the four waves of a workgroup have nothing in
//    common, so each wave walks its OWN stream of live code tiles (SliceFilterWindows, vg_slice_windows.hpp: a wave-uniform
//    bitmap of a window of 64 of the wave's tiles, one 8-byte load a lane at any alignment; a slice that sticks out of the
//    filter — the last row tile's — reads the filter's last 8 bytes and shifts, never past (n + 7) / 8; the launch takes this
//    variant from n = 64 up); a wave without one leaves behind that barrier.  The ring keeps flying across skipped tiles: the
//    last chunk's slots load the first chunk of the next LIVE tile, unconditionally as before, and that tile is found at the
//    tile's START, ahead of its chunks — scalar work (s_ff1 on the bitmap) while the window lasts.  The next window is loaded
//    when the current one is spent and waited for there (why not a window ahead: the note in vg_pq_small_gemm.hpp), a drain once
//    in 64 of the wave's tiles that lies between two tiles, where the chunk's-end copy has drained the ring anyway.  Read from
//    the ISA: the window's load and its vmcnt(0) stand in blocks ahead of the K loop only; the K loop's waits are vmcnt(20) per
//    step (Dot: 18) — the 16 pieces, the tile's two norms and the two filter bytes with a lane's rows' bits, loaded beside the
//    norms — and vmcnt(21) (19) between steps, i.e. the unfiltered waits two loads deeper; vmcnt(0) at a chunk's end and at the
//    appends as unfiltered.  Past its end the stream repeats the first chunk of the tile it is on — a walked one, in range.  A
//    walked tile's rows still test their own bit beside `row < n`; bits at or past n can make the last tile walked, never a row
//    appended.  Registers (profiles/kernel_resources.txt): at most 6 VGPRs above the unfiltered ones, no scratch; the Dot variants of
//    two query blocks take 194 / 196 VGPRs beside 64 AGPRs and lose the second workgroup a CU that 192 allowed.
//    Measured: the comment above kSq8NomCodesMaskedMinPairs (k_sq8_scan.hip).
// The error bound (Sq8CodesRow::eps, k_sq8_scan.hip, "GEMM sum"): that term allows a start at s (|s| <= 1.501 B for L2, 2.002 B for
// Dot), dim products (S = sum |products| <= 0.51 B) and the key's fma, (dim + 16) roundings of at most u (|s| + S) each whatever
// their order: 4.03 (dim + 16) u B for L2 (the score is twice the sum), 2.52 (dim + 16) u B for Dot.  This tile starts at ZERO: its
// dim roundings are of partial sums of at most S, 0.51 dim u B in the sum.  L2: 1.02 dim u B in the score, and the key's fma rounds
// a value of at most |x^|^2 + 2 S <= 2.02 B once: (1.02 dim + 2.02) u B, inside 4.03 (dim + 16) u B.  Dot: the key is -acc, a sign
// flip with no rounding: 0.51 dim u B, inside 2.52 (dim + 16) u B.  Both hold — eps is unchanged and Dot takes the tile too.
// Non-finite values: a NaN score is never below a threshold and is not appended; the proof fails on its margin as for the big tile.
//
// The limiter, and what was tried.  A lane converts 32 codes a step for 4 RB matrix instructions, so at RB = 1 the vector ALU has
// more cycles a step than the matrix unit.  The conversion as written costs 1.5 instructions a code: the compiler selects the
// signed byte INSIDE the convert (v_cvt_f32_i32 with an SDWA sext byte select — no v_bfe_i32) and packs two floats per
// v_cvt_pk_bf16_f32; read from the ISA.  v_cvt_f32_ubyteN followed by a subtraction of 128 is 2.5 a code and was not kept; a byte
// permute cannot build bf16(c - 128) (the normalisation is the conversion), and bf16(c) uncentred with a -128 sum(q) correction
// would leave the score space Sq8CodesRow::eps bounds.  Sharing a conversion between the two row blocks is not possible: they are
// different rows, and each code is converted exactly once as it is.  Measured (MI355X, dim 768, the GEMM's profile scope): 8
// queries x 1M rows 0.167 ms, 32: 0.168, 64: 0.195 — 4.6 TB/s of code bytes (5.6 TB/s at 10M rows): with 1.5 instructions a code
// the tile is HBM-bound at RB = 1 and 2, not VALU-bound; 96: 0.246, 128 (two launches): 0.384.  The whole table: the comment above kSq8NomCodesSmallMinPairs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "vg_device.hpp"
#include "vg_flat_gemm.hpp"
#include "vg_slice_windows.hpp"

namespace vg {

constexpr int kS8sThreads = 256, kS8sBN = 256, kS8sDepth = 8;
static_assert(kS8sBN == kSliceBN, "the filter windows' row tile is this tile's");
constexpr size_t kS8sLdsMax = 160 * 1024;  // a CU's LDS (gfx950)
// the 32-dimension steps of a row of `groups` 16-dimension groups
__host__ __device__ constexpr int sq8_small_steps(int groups) { return (groups + 1) >> 1; }
// the kernel's dynamic LDS for rb blocks of 32 queries: the image (four granules a step and query) and the thresholds
__host__ __device__ constexpr size_t sq8_small_lds_bytes(int rb, int groups)
{
    return static_cast<size_t>(sq8_small_steps(groups)) * 4 * 16 * (rb * 32) + sizeof(float) * (rb * 32);
}

// 8 codes with every byte's top bit flipped (x = bytes ^ 0x80) as their granule of 8 bfloat16: code - 128, the low byte first
__device__ __forceinline__ uint4 sq8_half_bf16(uint32_t lo, uint32_t hi)
{
    auto pair = [](uint32_t x, int at) {  // bytes at / 8 and at / 8 + 1 as signed bytes
        const float a = static_cast<float>(static_cast<int>(x << (24 - at)) >> 24), b = static_cast<float>(static_cast<int>(x << (16 - at)) >> 24);
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(vg_f32x2{a, b}, vg_bf16x2));
    };
    return make_uint4(pair(lo, 0), pair(lo, 16), pair(hi, 0), pair(hi, 16));
}

// queries: nq x dim_pad bfloat16 (gemm_operands' image scaled by the inverse scales, the tail from dim on zeros), nq <= 32 RB,
// dim_pad >= 32 steps; tiles: the index's code tiles, n_tiles = ceil(n / 64) of `groups` groups; counts: counts[q * count_stride];
// cand: cap keys a query; MASKED: mask, a bit per row, (n + 7) / 8 bytes at any alignment — BATCH: one for all queries (n >= 64: 8
// bytes of it exist), otherwise query q's at mask + q * mask_stride (a stride of 0: one for all, without the skip)
template <bool DOT, int RB, bool MASKED = false, bool BATCH = false>
__global__ __launch_bounds__(kS8sThreads) void flat_gemm_sq8_small_kernel(
    const uint16_t *__restrict__ queries, int nq, int dim_pad, const uint8_t *__restrict__ tiles, int64_t n, int groups,
    const float *__restrict__ norms, const float *__restrict__ thr, int thr_stride, int thr_off, int *__restrict__ counts, int count_stride,
    uint64_t *__restrict__ cand, int cap, const uint8_t *__restrict__ mask, int64_t mask_stride)
{
    static_assert(RB >= 1 && RB <= 4, "one to four blocks of 32 queries");
    static_assert(MASKED || !BATCH, "a batch filter is a filter");
    constexpr bool SKIP = MASKED && BATCH;
    constexpr int QB = RB * 32, D = kS8sDepth;
    extern __shared__ float gemm_lds[];
    const int ntiles = static_cast<int>((n + kS8sBN - 1) / kS8sBN), G = static_cast<int>(gridDim.x);
    if (static_cast<int>(blockIdx.x) >= ntiles) return;  // (the whole workgroup: nothing below is reached by a part of it)
    const int64_t last_ct = (n + 63) / 64 - 1;           // the last code tile that exists
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nsteps = sq8_small_steps(groups), nchunks = (nsteps + D - 1) / D;
    const bool odd = groups & 1;  // lane half 1 has no group in the last step
    uint4 *const img = reinterpret_cast<uint4 *>(gemm_lds);
    float *const lds_thr = gemm_lds + nsteps * 4 * QB * 4;

    // the image, once: granule g = ((i 2 + m) 2 + hh) QB + q <- dimensions 32 i + 16 hh + 8 m .. + 8 of query q (< dim_pad)
    for (int g = tid; g < nsteps * 4 * QB; g += kS8sThreads) {
        const int q = g % QB, x = g / QB, hh = x & 1, m = (x >> 1) & 1, i = x >> 2;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (q < nq) v = *reinterpret_cast<const uint4 *>(queries + static_cast<int64_t>(q) * dim_pad + 32 * i + 16 * hh + 8 * m);
        img[g] = v;
    }
    if (tid < QB) lds_thr[tid] = tid < nq ? thr[static_cast<int64_t>(tid) * thr_stride + thr_off] : -INFINITY;
    __syncthreads();

    // this lane's byte offset inside a step of its code tile (row block 0; block 1: + 512): group 2 i + h, row r — and inside the last
    // step of an odd group count, where lane half 1 re-reads group 2 i
    const uint32_t off_lane = static_cast<uint32_t>(h * 64 + r) * 16, off_last = odd ? static_cast<uint32_t>(r) * 16 : off_lane;
    // step i of row tile t (steps past the last: the last again), both row blocks
    auto load_step = [&](int t, int i, uint4 (&dst)[2]) {
        const int64_t ct = static_cast<int64_t>(t) * 4 + wave;
        const int ii = i < nsteps ? i : nsteps - 1;
        const uint8_t *p = tiles + ((ct < last_ct ? ct : last_ct) * groups + 2 * ii) * 1024;  // (wave-uniform)
        const uint32_t off = ii == nsteps - 1 ? off_last : off_lane;
#pragma unroll
        for (int j = 0; j < 2; j++) dst[j] = *reinterpret_cast<const uint4 *>(p + off + j * 512);
    };

    // SKIP: the wave's tiles by ordinal (tile blockIdx.x + ordinal G) and the filter's windows over them; otherwise an empty struct.
    // ord: the ordinal of the tile that is computed — fw.mine: the wave's stream has ended
    std::conditional_t<SKIP, SliceFilterWindows, SliceNoFilter> fw;
    int ord = 0, t = static_cast<int>(blockIdx.x);
    if constexpr (SKIP) {
        ord = fw.init(mask, n, ntiles, G, wave, lane);
        if (ord >= fw.mine) return;  // (the wave alone: there is no barrier behind the image's)
        t += ord * G;
    }

    f32x16 acc[RB][2];
    uint4 ring[D][2];
#pragma unroll
    for (int p = 0; p < D; p++) {
        load_step(t, p, ring[p]);
        __builtin_amdgcn_sched_barrier(0);  // (in the ring's order: the K loop waits for its slots by count)
    }
    auto more = [&]() {
        if constexpr (SKIP)
            return ord < fw.mine;
        else
            return t < ntiles;
    };
    while (more()) {
        const int64_t n0 = static_cast<int64_t>(t) * kS8sBN + wave * 64;
        // SKIP: the wave's next tile whose slice keeps a row, found BEFORE the tile's chunks (scalar work inside a window; the one
        // load and wait of a window's end lie here, ahead of the K loop) — the tile whose first chunk the last chunk's slots load.
        // Past the stream's end: this tile — a walked one, in range — again.
        int ord_next = 0, t_next = t + G;
        if constexpr (SKIP) {
            ord_next = fw.next_live(ord + 1);
            t_next = ord_next < fw.mine ? static_cast<int>(blockIdx.x) + ord_next * G : t;
        }
        float xn[2] = {0.0f, 0.0f};
        if (!DOT) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int64_t nn = n0 + j * 32 + r;
                xn[j] = norms[nn < n ? nn : n - 1];
            }
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
#pragma unroll
        for (int b = 0; b < RB; b++)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[b][j][e] = 0.0f;
        for (int c = 0; c < nchunks; c++) {
            // the chunk whose loads take the slots this one frees — of the next tile behind the last one; past the stream's end: the
            // last tile's first again, never multiplied
            const bool last = c + 1 == nchunks;
            const int tn = !last ? t : SKIP ? t_next : (t + G < ntiles ? t + G : ntiles - 1), cn = last ? 0 : c + 1;
#pragma unroll
            for (int p = 0; p < D; p++) {
                const int i = c * D + p;
                // the slot's codes are taken (centred, masked) before its next load is issued, the load before the matrix instructions
                // (a padded step is taken too; it is not multiplied)
                // lane half 1's group behind an odd count: zeros as operands — centred codes of 0 (a mask, not a branch per lane half)
                const uint32_t keep = odd && i == nsteps - 1 && h ? 0u : 0xFFFFFFFFu;
                uint4 fb[2][2];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const uint4 x = make_uint4((ring[p][j].x ^ 0x80808080u) & keep, (ring[p][j].y ^ 0x80808080u) & keep,
                                               (ring[p][j].z ^ 0x80808080u) & keep, (ring[p][j].w ^ 0x80808080u) & keep);
                    fb[j][0] = sq8_half_bf16(x.x, x.y), fb[j][1] = sq8_half_bf16(x.z, x.w);
                }
                __builtin_amdgcn_sched_barrier(0);
                load_step(tn, cn * D + p, ring[p]);
                __builtin_amdgcn_sched_barrier(0);
                if (i < nsteps) {  // (wave-uniform; no vector-memory operation inside)
                    const uint4 *pa = img + (i * 4 + h) * QB + r;
#pragma unroll
                    for (int m = 0; m < 2; m++) {
                        uint4 fa[RB];
#pragma unroll
                        for (int b = 0; b < RB; b++) fa[b] = pa[m * 2 * QB + b * 32];
#pragma unroll
                        for (int b = 0; b < RB; b++)
#pragma unroll
                            for (int j = 0; j < 2; j++)
                                acc[b][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(vg_bf16x8, fa[b]),
                                                                                   __builtin_bit_cast(vg_bf16x8, fb[j][m]), acc[b][j], 0, 0, 0);
                    }
                }
                // (a step at a time: left to itself the scheduler hoists every step's reads and conversions of the chunk and takes a
                // register for each)
                __builtin_amdgcn_sched_barrier(0);
            }
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
                        sc[4 * g + e] = DOT ? -acc[b][j][4 * g + e] : __builtin_fmaf(-2.0f, acc[b][j][4 * g + e], xn[j]);
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
