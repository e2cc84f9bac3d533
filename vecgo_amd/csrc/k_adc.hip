// k_adc.hip — PQ-ADC flat scan with fused top-k (flat/segment.go:476-483, :678-689,
// :714-721) for gfx950.
//
// HBM layout of the codes ("tiles"): the reference keeps codes row-major,
// codes[i*m:(i+1)*m].  A lane-per-row scan of that layout issues 16-byte loads at a
// 96-byte stride (48 partially used lines per wave-instruction).  set_pq_codes re-tiles
// once: tile t = rows [64t, 64t+64); within a tile, group g (16 consecutive
// sub-quantizers) of all 64 rows is contiguous:
//     byte address = ((t*G + g)*64 + lane)*16,   G = ceil(m/16)
// so every wave-level load is one fully coalesced 1 KiB request and the scan streams
// exactly N*G*16 bytes (= N*m when 16 | m).
//
// LDS bank conflicts: a 256-entry table row per sub-quantizer puts a wave's 64 random
// lookups on random banks (ds_read_b32: 32 lanes over 32 banks, ~3.4 cycles per 32-lane
// group instead of 1).  Full 16-wide groups therefore use a ROTATED image: lane i
// (r = i & 15) reads, in slot s, sub-quantizer l = (s + r) & 15 of the group, and the LUT is
// stored [g][c][l] so that bank = 16*(c & 1) + l — the 16 rotations of a 32-lane group never
// collide, only the two lanes sharing a rotation can (p = 1/2).  The code bytes are
// pre-rotated per lane at re-tile time so slot s is byte s of the lane's 16-byte word.
// The rotation does not change the arithmetic: slot s accumulates the same
// sub-quantizers (g ascending) as reference lane l = (s+r)&15, and the
// _mm512_reduce_add_ps tree (i,i+8),(i,i+4),(i,i+2),(0,1) is invariant under a cyclic
// rotation of its 16 inputs because fp32 addition is commutative.
//
// Per-row arithmetic = pqAdcLookupAvx512 (internal/simd/src/floats_avx512.c:135-167):
// 16 lane accumulators acc[l] += table[(16g+l)*256 + code[16g+l]] for g ascending, the
// _mm512_reduce_add_ps tree, then the m%16 tail added sequentially.  fp32 adds only.
//
// (The fan-in merge of the scan's partial lists: k_topk_merge.hip.  The opt-in batch nomination the driver tries first:
// k_pq_nominate.hip.)
#include <algorithm>

#include "vg_adc_row.hpp"
#include "vg_adc_wide.hpp"
#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_cand_replay.hpp"
#include "vg_nominate.hpp"
#include "vg_scan_slices.hpp"
#include "vg_search.hpp"

namespace vg {

// with more than two waves per SIMD the per-wave register budget is what counts: keep hipcc from hoisting
// the byte extraction of a whole tile (96 temporaries) above the lookups it feeds
#if defined(VG_ADC_FENCE) && VG_ADC_FENCE
#define VG_ADC_SCHED_FENCE __builtin_amdgcn_sched_barrier(0);
#else
#define VG_ADC_SCHED_FENCE
#endif
#ifndef VG_ADC_DEAL
#define VG_ADC_DEAL 1
#endif
#ifndef VG_ADC_WAVES
#define VG_ADC_WAVES 8
#endif
constexpr int kAdcWaves = VG_ADC_WAVES;       // 512 threads, one workgroup per CU (LDS holds the LUT):
                                              // 2 waves/SIMD leaves each wave 256 VGPRs for deep prefetch
constexpr int kAdcThreads = kAdcWaves * kWave;
constexpr int kAdcSyncEvery = 2;              // iterations between candidate-buffer checks
constexpr int kAdcBuf = 4096;                 // candidate keys in LDS (32 KiB)

__global__ void pq_retile_kernel(const uint8_t *__restrict__ codes, int64_t n, int m, int groups,
                                 int64_t n_tiles, uint4 *__restrict__ tiles)
{
    int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    int64_t total = n_tiles * groups * 64;
    if (gid >= total) return;
    int lane = static_cast<int>(gid & 63);
    int64_t tg = gid >> 6;
    int g = static_cast<int>(tg % groups);
    int64_t t = tg / groups;
    int64_t row = t * 64 + lane;
    uint32_t w[4] = {0, 0, 0, 0};
    if (row < n) {
        const uint8_t *src = codes + row * m + g * 16;
        int cnt = m - g * 16;
        if (cnt >= 16) {  // full group: slot s holds sub-quantizer (s + lane) & 15
            for (int b = 0; b < 16; b++)
                w[b >> 2] |= static_cast<uint32_t>(src[(b + lane) & 15]) << (8 * (b & 3));
        } else {          // m % 16 tail: natural order (summed sequentially)
            for (int b = 0; b < cnt; b++)
                w[b >> 2] |= static_cast<uint32_t>(src[b]) << (8 * (b & 3));
        }
    }
    tiles[gid] = make_uint4(w[0], w[1], w[2], w[3]);
}
// (vg_vamana_reorder_bfs rebuilds the tiles from its permuted row-major codes: k_vamana_reorder.hip)
int32_t launch_pq_retile(const uint8_t *codes, int64_t n, int m, int groups, int64_t n_tiles, uint8_t *tiles, hipStream_t st)
{
    const int64_t total = n_tiles * groups * 64;
    VG_LAUNCH(pq_retile_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st, codes, n, m, groups, n_tiles,
              reinterpret_cast<uint4 *>(tiles));
    return VG_OK;
}


// ---- hand-pipelined LDS gathers -------------------------------------------------------------
// hipcc waits after every few ds_read_b32 of an unrolled gather, which at 2 waves/SIMD leaves the
// LDS pipe mostly idle.  The scan issues each 16-lookup group as 16 back-to-back ds_read_b32 in
// inline asm and retires it with a COUNTED s_waitcnt while the next group's 16 reads are already
// in flight.  hipcc does not track asm loads: every value is an in/out operand of the wait
// statement, so no consumer can be scheduled above it (cdna_hip_programming.md §5.7).
struct Vals8 {
    float v[8];
};

template <int OFF>
__device__ __forceinline__ float lds_read_off(uint32_t addr)
{
    float v;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}

// wait until at most N (<= 15: lgkmcnt is 4 bits) LGKM operations are outstanding; ties the 8
// values to the wait so no consumer can move above it
template <int N>
__device__ __forceinline__ void lds_wait(Vals8 &x)
{
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(x.v[0]), "+v"(x.v[1]), "+v"(x.v[2]), "+v"(x.v[3]), "+v"(x.v[4]),
                   "+v"(x.v[5]), "+v"(x.v[6]), "+v"(x.v[7])
                 : "n"(N));
}

// issue 8 rotated lookups (half H of group G) for code word c: slot s reads the pair-interleaved
// image at byte (G>>1)*32768 + code*128 + (G&1)*64 + rotoff[s]
template <int G, int H>
__device__ __forceinline__ void issue_half(Vals8 &dst, const uint4 &c, const uint32_t (&rotoff)[16])
{
    // ds offsets are 16-bit: groups 4+ go through a base bumped by 64 KiB
    constexpr int OFF = ((G >> 1) & 1) * 32768 + (G & 1) * 64;
    constexpr uint32_t BUMP = (G >> 2) * 65536u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int sl = H * 8 + i;
        const uint32_t addr = (code_byte(c, sl) << 7) + rotoff[sl] + BUMP;
#ifdef VG_ADC_PROBE_NO_LDS   // stage probe (tools/build_variant.sh): the address arithmetic without the lookup
        dst.v[i] = __uint_as_float(addr + OFF);
#else
        dst.v[i] = lds_read_off<OFF>(addr);
#endif
    }
}

template <int H>
__device__ __forceinline__ void accumulate_half(float (&acc)[16], const Vals8 &x)
{
#pragma unroll
    for (int i = 0; i < 8; i++) acc[H * 8 + i] = acc[H * 8 + i] + x.v[i];
}

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ bool span_nonempty(int64_t t0, int64_t t1) { return t1 > t0; }

struct AdcShared {
    // dynamic LDS: float lut[m*256]; uint64 buf[kAdcBuf]; then these words
    int cnt;
    int pad;
    uint64_t tau;
};

// GF = number of full 16-wide groups when known at compile time (m = 16*GF exactly),
// or -1 for the generic shape (runtime full groups + tail).
// SMALLK: k <= 64 — each wave keeps its top-k in registers (WaveTopK) and the scan loop has
// no workgroup barrier; otherwise candidates go through the shared LDS buffer.
// ONCE: one query per pass — nobody re-reads the codes, so they are streamed (load_stream); with several
// queries the blocks of an XCD share a slice through L2 and the loads stay plain.
// MASKED (SMALLK only): the filtered search of k_probe.hip — a row the query's filter rejects offers no key; desc: a Dot /
// Cosine segment keeps the LARGEST lookups (flat/segment.go:449).  A template flag: the unfiltered scans stay as they were.
// PROBED (SMALLK only): the partition-probed scan (flat/segment.go:727-744) — workgroup (query q, share s of `slices`) walks the
// tile ranges of probes s, s + slices, ... of its query with the same pipelined loop, rows outside a partition's range masked
// (partition bounds are not tile-aligned); min_keys: paged results.  (r05 ran these through a plain gather loop: 2x the time.)
template <int GF, bool SMALLK, bool ONCE, bool MASKED = false, bool PROBED = false>
__global__ __launch_bounds__(kAdcThreads) void pq_adc_scan_kernel(
    const uint4 *__restrict__ tiles, int64_t n_rows, int64_t n_tiles, int m, int groups,
    const float *__restrict__ tables, int slices, int nq, int k, uint64_t *__restrict__ partial,
    int raw_lists, const int *__restrict__ only_if, const uint8_t *__restrict__ mask, int64_t mask_stride, bool desc,
    const uint32_t *__restrict__ probes = nullptr, const uint32_t *__restrict__ part_off = nullptr, int np = 0,
    const uint64_t *__restrict__ min_keys = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *lut = reinterpret_cast<float *>(smem);
    const int lut_words = lut_image_words(m);
    const int lut_tail_word = (((m >> 4) + 1) >> 1) * 8192;
    uint64_t *buf = reinterpret_cast<uint64_t *>(smem + static_cast<size_t>(lut_words) * sizeof(float));
    AdcShared *sh = reinterpret_cast<AdcShared *>(buf + kAdcBuf);

    // XCD-aware mapping: blocks b and b+8 share an XCD (and its L2).  Consecutive blocks of
    // one XCD take different queries over the SAME row slice, so the slice is fetched from
    // HBM once per XCD and served to the other queries from that XCD's L2.
    const int b = blockIdx.x;
    const int xcd = b & 7;
    const int o = b >> 3;
    const int q = PROBED ? b / slices : o % nq;
    const int s = PROBED ? b % slices : (o / nq) * 8 + xcd;
    if (only_if && !only_if[q]) return;  // fallback launch: only the flagged queries run
    int64_t t0 = n_tiles * s / slices;
    int64_t t1 = n_tiles * (s + 1) / slices;
    int64_t R0 = 0, R1 = n_rows;  // PROBED: the probed partition's rows
    const uint8_t *mq = MASKED && mask ? mask + static_cast<int64_t>(q) * mask_stride : nullptr;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int rot = lane & 15;
    const float *lut_rot = lut;  // full groups: [g][c][l]; tail rows follow in [j][c] order

    {   // stage this query's lookup table (m KiB) into LDS with 16-byte loads
        const float4 *src = reinterpret_cast<const float4 *>(tables + static_cast<int64_t>(q) * lut_words);
        float4 *dst = reinterpret_cast<float4 *>(lut);
        // 4 independent 16-byte loads in flight per thread.  No per-load guards: a guarded load
        // makes hipcc branch around it and wait vmcnt(0) each time (serialized L2 round trips).
        const int n4 = lut_words / 4;
        const int rounds = n4 / kAdcThreads;
        int r = 0;
        for (; r + 4 <= rounds; r += 4) {
            float4 tmp[4];
#pragma unroll
            for (int u = 0; u < 4; u++) tmp[u] = src[(r + u) * kAdcThreads + tid];
#pragma unroll
            for (int u = 0; u < 4; u++) dst[(r + u) * kAdcThreads + tid] = tmp[u];
        }
        for (int i = r * kAdcThreads + tid; i < n4; i += kAdcThreads) dst[i] = src[i];
    }
    if (tid == 0) {
        sh->cnt = 0;
        sh->tau = kKeyMax;
    }
    __syncthreads();
    uint64_t tau = kKeyMax;
    WaveTopK wtk;
    wtk.init(raw_lists ? 64 : k);  // raw mode: every wave keeps its 64 best whatever k is

    const int gfull = (GF >= 0) ? GF : (m >> 4);
    const int tail = (GF >= 0) ? 0 : (m & 15);
    // Which tiles a workgroup takes.  Several queries per pass: a contiguous slice [t0, t1), so that the blocks of
    // an XCD re-read one slice through their L2.  One query per pass (ONCE): the tiles are dealt round-robin over
    // the workgroups — trip `it` of workgroup s, wave w is tile (it * slices + s) * waves + w — so that at any
    // moment the whole chip streams ONE moving window of the code array instead of `slices` distant ones (DRAM
    // pages stay open, the stream runs at the rate of a plain sequential read).
    constexpr bool kDealt = ONCE && VG_ADC_DEAL && !PROBED;
    for (int jr = PROBED ? s : 0; jr < (PROBED ? np : 1); jr += PROBED ? slices : 1) {
    if (PROBED) {
        const uint32_t pp = probes[static_cast<int64_t>(q) * np + jr];
        R0 = part_off[pp];
        R1 = part_off[pp + 1];
        t0 = R0 >> 6;
        t1 = (R1 + 63) >> 6;
    }
    const int64_t tstride = kDealt ? static_cast<int64_t>(slices) * kAdcWaves : kAdcWaves;
    const int64_t tbase = kDealt ? static_cast<int64_t>(s) * kAdcWaves : t0;
    const int64_t tend = kDealt ? n_tiles : t1;
    const int64_t span = tend - tbase;
    const int iters = span > 0 ? static_cast<int>((span + tstride - 1) / tstride) : 0;

    // software pipeline: the next tile's 16-byte code words are in flight while this
    // tile's lookups run (GF known at compile time)
    uint4 nxt[GF > 0 ? GF : 1];
    // m = 96 single-query passes keep two tiles in flight per wave when the workgroup has 8 waves (256 VGPRs
    // each); with more waves per SIMD the same bytes are in flight one tile ahead
    constexpr bool kTwoAhead = GF == 6 && ONCE && kAdcWaves <= 8;
    uint4 nxt2[kTwoAhead ? 6 : 1];
    uint32_t rotoff[16];
#pragma unroll
    for (int sl = 0; sl < 16; sl++) rotoff[sl] = static_cast<uint32_t>(((sl + rot) & 15) * 4);
    // Prefetch loads are UNGUARDED (a guarded load makes hipcc wait vmcnt(0) at the join): past
    // the end of the slice the address is clamped to the slice's last tile and the data unused.
    const int64_t tlast = tend - 1;
    if (GF > 0 && span > 0) {
        const int64_t tile0 = min64(tbase + wave, tlast);
        const uint4 *tp0 = tiles + (tile0 * groups) * 64 + lane;
#pragma unroll
        for (int g = 0; g < GF; g++) nxt[g] = ONCE ? load_stream(tp0 + g * 64) : tp0[g * 64];
        if (kTwoAhead) {
            const int64_t tile1 = min64(tbase + wave + tstride, tlast);
            const uint4 *tp1 = tiles + (tile1 * groups) * 64 + lane;
#pragma unroll
            for (int g = 0; g < 6; g++) nxt2[g] = load_stream(tp1 + g * 64);
        }
    }
    for (int it = 0; it < iters; it++) {
        const int64_t tile = tbase + static_cast<int64_t>(it) * tstride + wave;
        if (tile < tend) {
            const uint4 *tp = tiles + (tile * groups) * 64 + lane;
            float acc[16];
#pragma unroll
            for (int l = 0; l < 16; l++) acc[l] = 0.0f;
            if (GF == 6) {
                uint4 c[6];
#pragma unroll
                for (int g = 0; g < 6; g++) c[g] = nxt[g];
                if (kTwoAhead) {  // two tiles ahead: ~96 KiB of code loads in flight per CU instead of 48
                    const int64_t tile2 = min64(tile + 2 * tstride, tlast);
                    const uint4 *tn = tiles + (tile2 * groups) * 64 + lane;
#pragma unroll
                    for (int g = 0; g < 6; g++) {
                        nxt[g] = nxt2[g];
                        nxt2[g] = load_stream(tn + g * 64);
                    }
                } else {
                    const int64_t tile1 = min64(tile + tstride, tlast);
                    const uint4 *tn = tiles + (tile1 * groups) * 64 + lane;
#pragma unroll
                    for (int g = 0; g < 6; g++) nxt[g] = ONCE ? load_stream(tn + g * 64) : tn[g * 64];
                }
#ifdef VG_ADC_PROBE_NO_HBM   // stage probe: every tile re-uses the first tile's code words (no loads in the loop)
#pragma unroll
                for (int g = 0; g < 6; g++) {
                    nxt[g] = c[g];
                    if (kTwoAhead) nxt2[g] = c[g];
                }
#endif
                // two register sets ping-pong: the next 8 lookups are in flight while the
                // previous 8 retire (same order of additions per slot: g ascending)
                Vals8 va, vb;
                issue_half<0, 0>(va, c[0], rotoff);
#define VG_STEP(GA, HA, GB, HB, X, Y)            \
    issue_half<GB, HB>(Y, c[GB], rotoff);        \
    lds_wait<8>(X);                              \
    accumulate_half<HA>(acc, X);                 \
    VG_ADC_SCHED_FENCE
                VG_STEP(0, 0, 0, 1, va, vb)
                VG_STEP(0, 1, 1, 0, vb, va)
                VG_STEP(1, 0, 1, 1, va, vb)
                VG_STEP(1, 1, 2, 0, vb, va)
                VG_STEP(2, 0, 2, 1, va, vb)
                VG_STEP(2, 1, 3, 0, vb, va)
                VG_STEP(3, 0, 3, 1, va, vb)
                VG_STEP(3, 1, 4, 0, vb, va)
                VG_STEP(4, 0, 4, 1, va, vb)
                VG_STEP(4, 1, 5, 0, vb, va)
                VG_STEP(5, 0, 5, 1, va, vb)
#undef VG_STEP
                lds_wait<0>(vb);
                accumulate_half<1>(acc, vb);
            } else if (GF >= 0) {
                uint4 c[GF > 0 ? GF : 1];
#pragma unroll
                for (int g = 0; g < GF; g++) c[g] = nxt[g];
                {
                    const int64_t tile1 = min64(tile + tstride, tlast);
                    const uint4 *tn = tiles + (tile1 * groups) * 64 + lane;
#pragma unroll
                    for (int g = 0; g < GF; g++) nxt[g] = ONCE ? load_stream(tn + g * 64) : tn[g * 64];
                }
#pragma unroll
                for (int g = 0; g < GF; g++) {
#pragma unroll
                    for (int sl = 0; sl < 16; sl++)
                        acc[sl] = acc[sl] + lut_rot[((g >> 1) * 256 + code_byte(c[g], sl)) * 32 + (g & 1) * 16 + ((sl + rot) & 15)];
                }
            } else {
                for (int g = 0; g < gfull; g++) {
                    uint4 c = tp[g * 64];
#pragma unroll
                    for (int sl = 0; sl < 16; sl++)
                        acc[sl] = acc[sl] + lut_rot[((g >> 1) * 256 + code_byte(c, sl)) * 32 + (g & 1) * 16 + ((sl + rot) & 15)];
                }
            }
            float total = reduce16_regs(acc);
            if (tail) {
                uint4 c = tp[gfull * 64];
                for (int l = 0; l < tail; l++)
                    total = total + lut[lut_tail_word + l * 256 + code_byte(c, l)];
            }
            const int64_t row = tile * 64 + lane;
            uint64_t key;
            if constexpr (MASKED || PROBED) {
                const bool live = row < n_rows && (!PROBED || (row >= R0 && row < R1)) && (!MASKED || mask_bit(mq, row));
                key = live ? make_key(total, static_cast<uint32_t>(row), desc) : kKeyMax;
                if (PROBED && min_keys && key <= min_keys[q]) key = kKeyMax;  // paged results (k > 64)
            } else {
                key = (row < n_rows) ? make_key(total, static_cast<uint32_t>(row), false) : kKeyMax;
            }
            if (SMALLK) {
                wtk.offer(key, lane);
            } else if (key < tau) {
                int pos = atomicAdd(&sh->cnt, 1);
                buf[pos] = key;  // pos < kAdcBuf by the sync protocol below
            }
        }
        if (SMALLK) continue;
        // Every kAdcSyncEvery iterations at most kAdcSyncEvery*1024 keys were appended;
        // compact when the next round could overflow the buffer.
        if ((it % kAdcSyncEvery) == kAdcSyncEvery - 1 || it == iters - 1) {
            __syncthreads();
            int c = sh->cnt;
            const bool last = (it == iters - 1);
            if (last || c > kAdcBuf - kAdcSyncEvery * kAdcThreads) {
                for (int i = c + tid; i < kAdcBuf; i += kAdcThreads) buf[i] = kKeyMax;
                __syncthreads();
                bitonic_sort_lds(buf, kAdcBuf, tid, kAdcThreads);
                if (tid == 0) {
                    int keep = c < k ? c : k;
                    sh->cnt = keep;
                    sh->tau = (c >= k) ? buf[k - 1] : kKeyMax;
                }
                __syncthreads();
            }
            tau = sh->tau;
        }
    }
    }  // probed ranges
    if (SMALLK && raw_lists) {
        partial[((static_cast<int64_t>(q) * slices + s) * kAdcWaves + wave) * 64 + lane] = wtk.list;
        return;
    }
    uint64_t *out = partial + (static_cast<int64_t>(q) * slices + s) * k;
    if (SMALLK) {
        wg_rank_merge<kAdcWaves>(wtk, buf, reinterpret_cast<int *>(buf + kAdcWaves * 64), wave, lane,
                                 tid, k, out);
        return;
    }
    const int have = sh->cnt;
    for (int i = tid; i < k; i += kAdcThreads) out[i] = (i < have) ? buf[i] : kKeyMax;
}

// (r01/r02 carried a second m = 96 kernel here, `pq_adc_scan96_kernel`: 16-lane halves of a wave one group apart so
// that no two lanes of a 32-lane LDS group share a bank — 25 lookups per clock and CU in the microbenchmark against
// 15 for the rotated image below.  Bit-exact, but its lane-dependent address selects cost ~7 vector instructions per
// lookup and it never won: 70 k vs 82 k queries/s at 1M rows (r01), and on the LDS-bound batch of r03 — 64 queries x
// 10M rows — 7.0 k vs 8.2 k queries/s.  The one-query scan is bound by the HBM stream, not by LDS (r02 stage probes,
// DESIGN.md section 4), so there was nothing for it to win there either.  Dropped in r03.)

// k > 64: per query, the k best keys of the union of `lists` per-wave lists (64 keys each,
// ascending, kKeyMax padded) and a proof that nothing better was dropped: a wave only ever
// discards keys above its own 64th key, so the result is exact iff the k-th selected key is not
// above T = min over FULL lists of their 64th key.  flag[q] = 1 asks for the exhaustive path.
__global__ __launch_bounds__(kMergeThreads) void topk_select_verify_kernel(
    const uint64_t *__restrict__ raw, int lists, int k, bool descending, uint32_t *__restrict__ ids,
    float *__restrict__ scores, int *__restrict__ flags)
{
    __shared__ uint64_t buf[kMergeBuf];
    __shared__ unsigned long long tsafe;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const uint64_t *src = raw + q * lists * 64;
    const int64_t total = static_cast<int64_t>(lists) * 64;
    if (tid == 0) tsafe = kKeyMax;
    __syncthreads();
    uint64_t t = kKeyMax;
    for (int l = tid; l < lists; l += kMergeThreads) {
        const uint64_t v = src[static_cast<int64_t>(l) * 64 + 63];
        t = v < t ? v : t;
    }
    if (t != kKeyMax) atomicMin(&tsafe, static_cast<unsigned long long>(t));
    __shared__ int cnt;
    __shared__ unsigned long long tcut_s;
    bool done = false;
    if (total > kMergeBuf && lists <= kMergeBuf) {
        // Prune before sorting.  An upper bound on the k-th smallest key of the union:
        //   lists >= k : the k-th smallest list HEAD (k distinct keys are <= it)
        //   otherwise  : max_l list_l[j-1], j = ceil(k / lists) (the first j of every list are k keys)
        uint64_t tcut;
        if (lists >= k) {
            for (int i = tid; i < kMergeBuf; i += kMergeThreads)
                buf[i] = i < lists ? src[static_cast<int64_t>(i) * 64] : kKeyMax;
            __syncthreads();
            bitonic_sort_lds(buf, kMergeBuf, tid, kMergeThreads);
            tcut = buf[k - 1];
            __syncthreads();
        } else {
            const int j = (k + lists - 1) / lists;  // <= 64 because k <= lists * 64 is checked by the host
            if (tid == 0) tcut_s = 0;
            __syncthreads();
            uint64_t mx = 0;
            for (int l = tid; l < lists; l += kMergeThreads) {
                const uint64_t v = src[static_cast<int64_t>(l) * 64 + (j - 1)];
                mx = v > mx ? v : mx;
            }
            atomicMax(&tcut_s, static_cast<unsigned long long>(mx));
            __syncthreads();
            tcut = tcut_s;
        }
        if (tid == 0) cnt = 0;
        __syncthreads();
        for (int l = tid; l < lists; l += kMergeThreads) {  // lists are ascending: stop at the cut
            const uint64_t *lp = src + static_cast<int64_t>(l) * 64;
            for (int i = 0; i < 64; i++) {
                const uint64_t key = lp[i];
                if (key == kKeyMax || key > tcut) break;
                const int p = atomicAdd(&cnt, 1);
                if (p < kMergeBuf) buf[p] = key;
            }
        }
        __syncthreads();
        const int c = cnt;
        if (c <= kMergeBuf) {
            for (int i = c + tid; i < kMergeBuf; i += kMergeThreads) buf[i] = kKeyMax;
            __syncthreads();
            bitonic_sort_lds(buf, kMergeBuf, tid, kMergeThreads);
            done = true;
        }
        __syncthreads();
    }
    if (!done) {
        int kept = 0;
        int64_t pos = 0;
        do {
            const int room = kMergeBuf - kept;
            const int take = static_cast<int>((total - pos) < room ? (total - pos) : room);
            for (int i = tid; i < take; i += kMergeThreads) buf[kept + i] = src[pos + i];
            for (int i = kept + take + tid; i < kMergeBuf; i += kMergeThreads) buf[i] = kKeyMax;
            __syncthreads();
            bitonic_sort_lds(buf, kMergeBuf, tid, kMergeThreads);
            pos += take;
            kept = k;
        } while (pos < total);
    }
    const uint64_t T = tsafe;
    const uint64_t kth = buf[k - 1];
    if (tid == 0) flags[q] = (T == kKeyMax || (kth != kKeyMax && kth <= T)) ? 0 : 1;
    for (int i = tid; i < k; i += kMergeThreads) {
        const uint64_t e = buf[i];
        ids[q * k + i] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        scores[q * k + i] = e == kKeyMax ? (descending ? -INFINITY : INFINITY) : key_score(e, descending);
    }
}

__global__ void patch_results_kernel(const int *__restrict__ flags, int k, const uint32_t *__restrict__ fids,
                                     const float *__restrict__ fscores, uint32_t *__restrict__ ids,
                                     float *__restrict__ scores)
{
    const int64_t q = blockIdx.x;
    if (!flags[q]) return;
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        ids[q * k + i] = fids[q * k + i];
        scores[q * k + i] = fscores[q * k + i];
    }
}


// ---- partition-probed ADC scan (flat/segment.go:727-744 over the :678-689 branch) -----------------
// One workgroup per (query, share of its probe list): the query's table is staged once, then the
// tiles covering each probed partition's row range [R0, R1) are scanned with the rows outside the
// range masked (partition bounds are not tile-aligned).  A few thousand rows per partition: the
// plain gather loop, no hand pipelining.  k <= 64.
__global__ __launch_bounds__(kAdcThreads) void pq_adc_probe_kernel(
    const uint4 *__restrict__ tiles, int64_t n_rows, int m, int groups, const float *__restrict__ tables,
    const uint32_t *__restrict__ probes, const uint32_t *__restrict__ part_off, int np, int split, int k,
    uint64_t *__restrict__ partial, const uint64_t *__restrict__ min_keys, bool desc, const uint8_t *__restrict__ mask,
    int64_t mask_stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *lut = reinterpret_cast<float *>(smem);
    const int lut_words = lut_image_words(m);
    uint64_t *buf = reinterpret_cast<uint64_t *>(smem + static_cast<size_t>(lut_words) * sizeof(float));
    const int y = blockIdx.x;
    const int64_t q = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rot = lane & 15;
    {
        const float4 *src = reinterpret_cast<const float4 *>(tables + q * lut_words);
        float4 *dst = reinterpret_cast<float4 *>(lut);
        const int n4 = lut_words / 4;
        const int rounds = n4 / kAdcThreads;
        int r = 0;
        for (; r + 4 <= rounds; r += 4) {
            float4 tmp[4];
#pragma unroll
            for (int u = 0; u < 4; u++) tmp[u] = src[(r + u) * kAdcThreads + tid];
#pragma unroll
            for (int u = 0; u < 4; u++) dst[(r + u) * kAdcThreads + tid] = tmp[u];
        }
        for (int i = r * kAdcThreads + tid; i < n4; i += kAdcThreads) dst[i] = src[i];
    }
    __syncthreads();
    const uint8_t *mq = mask ? mask + q * mask_stride : nullptr;  // filter.Matches (segment.go:631-635)
    WaveTopK wtk;
    wtk.init(k);
    for (int j = y; j < np; j += split) {
        const uint32_t p = probes[q * np + j];
        const int64_t R0 = part_off[p], R1 = part_off[p + 1];
        const int64_t tt0 = R0 >> 6, tt1 = (R1 + 63) >> 6;
        for (int64_t tile = tt0 + wave; tile < tt1; tile += kAdcWaves) {
            const uint4 *tp = tiles + (tile * groups) * 64 + lane;
            const int64_t row = tile * 64 + lane;
            const bool live = row >= R0 && row < R1 && row < n_rows && mask_bit(mq, row);
            if (mq && !__any(live)) continue;  // a tile the filter leaves nothing of: its codes are not read
            const float total = adc_row_score_lds(lut, tp, m, rot);
            uint64_t key = live ? make_key(total, static_cast<uint32_t>(row), desc) : kKeyMax;
            if (min_keys && key <= min_keys[q]) key = kKeyMax;  // paged results (k > 64)
            wtk.offer(key, lane);
        }
    }
    wg_rank_merge<kAdcWaves>(wtk, buf, reinterpret_cast<int *>(buf + kAdcWaves * 64), wave, lane, tid, k,
                             partial + (q * split + y) * k);
}

static int32_t launch_probe_scan_adc_wide(const vg_index *idx, const float *tables, const uint32_t *probes, const uint32_t *part_off,
                                          int64_t nq, int np, int split, int k, uint64_t *partial, const uint64_t *min_keys, bool desc,
                                          const uint8_t *mask, int64_t mask_stride, hipStream_t st);

int32_t launch_probe_scan_adc(const vg_index *idx, const float *tables, const uint32_t *probes, const uint32_t *part_off,
                              int64_t nq, int np, int split, int k, uint64_t *partial, const uint64_t *min_keys, bool desc,
                              const uint8_t *mask, int64_t mask_stride, hipStream_t st)
{
    const vg_pq *pq = idx->pq;
    const size_t scan_lds = static_cast<size_t>(lut_image_words(pq->m)) * sizeof(float) + kAdcBuf * sizeof(uint64_t) + sizeof(AdcShared);
    const size_t lds = static_cast<size_t>(lut_image_words(pq->m)) * sizeof(float) + kAdcWaves * 64 * sizeof(uint64_t) + 64;
    // a table neither kernel below holds in LDS (m >= 144): walked in chunks (test hook kHookAdcWideAlways: whatever m is)
    if (lds > 160 * 1024 || hook(kHookAdcWideAlways))
        return launch_probe_scan_adc_wide(idx, tables, probes, part_off, nq, np, split, k, partial, min_keys, desc, mask, mask_stride, st);
    // a table that fits LDS next to the scan kernel's buffers, k <= 64: the pipelined scan kernel over the probed ranges
    if (k <= 64 && scan_lds <= 160 * 1024 && !hook(kHookProbeNoGroup)) {
        auto pick = [&](auto masked_tag) {
            constexpr bool M = decltype(masked_tag)::value;
            return pq->m == 96 ? pq_adc_scan_kernel<6, true, false, M, true> : pq_adc_scan_kernel<-1, true, false, M, true>;
        };
        auto kern = mask ? pick(std::true_type{}) : pick(std::false_type{});
        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(scan_lds)));
        const int64_t max_q = (int64_t(1) << 30) / split;
        for (int64_t q0 = 0; q0 < nq; q0 += max_q) {
            const int64_t cnt = nq - q0 < max_q ? nq - q0 : max_q;
            ProfScope prof(idx->ctx, "pq_adc_probe", st);
            VG_LAUNCH(kern, dim3(static_cast<unsigned>(cnt * split)), dim3(kAdcThreads), scan_lds, st,
                      reinterpret_cast<const uint4 *>(idx->d_pq_tiles), idx->n, idx->n_tiles, pq->m, idx->pq_groups,
                      tables + q0 * lut_image_words(pq->m), split, static_cast<int>(cnt), k, partial + q0 * split * k, 0, nullptr,
                      mask ? mask + q0 * mask_stride : nullptr, mask_stride, desc, probes + q0 * np, part_off, np,
                      min_keys ? min_keys + q0 : nullptr);
        }
        return VG_OK;
    }
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pq_adc_probe_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    for (int64_t q0 = 0; q0 < nq; q0 += 65535) {
        const int64_t cnt = nq - q0 < 65535 ? nq - q0 : 65535;
        ProfScope prof(idx->ctx, "pq_adc_probe", st);
        VG_LAUNCH(pq_adc_probe_kernel, dim3(static_cast<unsigned>(split), static_cast<unsigned>(cnt)), dim3(kAdcThreads),
                  lds, st, reinterpret_cast<const uint4 *>(idx->d_pq_tiles), idx->n, pq->m, idx->pq_groups,
                  tables + q0 * lut_image_words(pq->m), probes + q0 * np, part_off, np, split, k,
                  partial + q0 * split * k, min_keys ? min_keys + q0 : nullptr, desc, mask ? mask + q0 * mask_stride : nullptr,
                  mask_stride);
    }
    return VG_OK;
}

template <int GF, bool SMALLK>
static int32_t launch_scan(const vg_index *idx, const float *tables, int64_t nq, int k,
                           int slices, uint64_t *partial, hipStream_t st, int raw_lists = 0,
                           const int *only_if = nullptr, const uint8_t *mask = nullptr, int64_t mask_stride = 0,
                           bool desc = false)
{
    const vg_pq *pq = idx->pq;
    size_t lds = static_cast<size_t>(lut_image_words(pq->m)) * sizeof(float) + kAdcBuf * sizeof(uint64_t) +
                 sizeof(AdcShared);
    auto kern = nq == 1 ? pq_adc_scan_kernel<GF, SMALLK, true> : pq_adc_scan_kernel<GF, SMALLK, false>;
    if (SMALLK && (mask || desc)) kern = nq == 1 ? pq_adc_scan_kernel<GF, SMALLK, true, SMALLK> : pq_adc_scan_kernel<GF, SMALLK, false, SMALLK>;
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    // grid.x limit is 2^31-1; chunk the queries if needed
    const int64_t max_q = (1ll << 30) / slices;
    for (int64_t q0 = 0; q0 < nq; q0 += max_q) {
        int64_t cnt = nq - q0 < max_q ? nq - q0 : max_q;
        ProfScope prof(idx->ctx, "pq_adc_scan", st);
        VG_LAUNCH(kern, dim3(static_cast<unsigned>(cnt * slices)), dim3(kAdcThreads), lds,
                           st, reinterpret_cast<const uint4 *>(idx->d_pq_tiles), idx->n,
                           idx->n_tiles, pq->m, idx->pq_groups,
                           tables + q0 * lut_image_words(pq->m), slices, static_cast<int>(cnt), k,
                           partial + q0 * slices * (raw_lists ? kAdcWaves * 64 : k), raw_lists,
                           only_if ? only_if + q0 : nullptr, mask ? mask + q0 * mask_stride : nullptr, mask_stride, desc,
                           static_cast<const uint32_t *>(nullptr), static_cast<const uint32_t *>(nullptr), 0,
                           static_cast<const uint64_t *>(nullptr));
    }
    return VG_OK;
}

// ---------------------------------------------------------------------------------------------
// m above what one LDS image holds (m > 96 with the top-k buffers): the table walked in 96 KiB chunks for a batch of kWideTiles
// tiles per wave — adc_wide_walk, vg_adc_wide.hpp.  k <= 64 per launch.
// ---------------------------------------------------------------------------------------------
constexpr size_t kWideLdsBytes = kWideLdsWords * sizeof(float) + kAdcWaves * 64 * sizeof(uint64_t) + 64;  // the walker's, then wg_rank_merge's

// the unfiltered whole segment: workgroup (query q, slice s) as in pq_adc_scan_kernel
__global__ __launch_bounds__(kAdcThreads) void pq_adc_scan_wide_kernel(
    const uint4 *__restrict__ tiles, int64_t n_rows, int64_t n_tiles, int m, int groups,
    const float *__restrict__ tables, int slices, int nq, int k, uint64_t *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *lut = reinterpret_cast<float *>(smem);
    uint64_t *buf = reinterpret_cast<uint64_t *>(lut + kWideLdsWords);
    const int b = blockIdx.x;
    const int xcd = b & 7, o = b >> 3;
    const int q = o % nq;
    const int s = (o / nq) * 8 + xcd;
    const int64_t t0 = n_tiles * s / slices, t1 = n_tiles * (s + 1) / slices;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *image = tables + static_cast<int64_t>(q) * lut_image_words(m);
    WaveTopK wtk;
    wtk.init(k);
    for (int64_t b0 = t0; b0 < t1; b0 += static_cast<int64_t>(kAdcWaves) * kWideTiles) {
        bool want[kWideTiles];
        float total[kWideTiles];
#pragma unroll
        for (int tb = 0; tb < kWideTiles; tb++) want[tb] = b0 + static_cast<int64_t>(tb) * kAdcWaves + wave < t1;
        adc_wide_walk<kAdcWaves>(tiles, groups, m, image, lut, b0, want, tid, total);
#pragma unroll
        for (int tb = 0; tb < kWideTiles; tb++) {
            const int64_t row = (b0 + static_cast<int64_t>(tb) * kAdcWaves + wave) * 64 + lane;
            wtk.offer(want[tb] && row < n_rows ? make_key(total[tb], static_cast<uint32_t>(row), false) : kKeyMax, lane);
        }
    }
    __syncthreads();
    uint64_t *out = partial + (static_cast<int64_t>(q) * slices + s) * k;
    wg_rank_merge<kAdcWaves>(wtk, buf, reinterpret_cast<int *>(buf + kAdcWaves * 64), wave, lane, tid, k, out);
}

// pq_adc_probe_kernel over such a table (same arguments, same grid): the tiles covering each probed range in batches, a tile
// outside the range or that the filter leaves no row of not wanted
__global__ __launch_bounds__(kAdcThreads) void pq_adc_probe_wide_kernel(
    const uint4 *__restrict__ tiles, int64_t n_rows, int m, int groups, const float *__restrict__ tables,
    const uint32_t *__restrict__ probes, const uint32_t *__restrict__ part_off, int np, int split, int k,
    uint64_t *__restrict__ partial, const uint64_t *__restrict__ min_keys, bool desc, const uint8_t *__restrict__ mask,
    int64_t mask_stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *lut = reinterpret_cast<float *>(smem);
    uint64_t *buf = reinterpret_cast<uint64_t *>(lut + kWideLdsWords);
    const int y = blockIdx.x;
    const int64_t q = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *image = tables + q * lut_image_words(m);
    const uint8_t *mq = mask ? mask + q * mask_stride : nullptr;  // filter.Matches (segment.go:631-635)
    const uint64_t floor_key = min_keys ? min_keys[q] : 0;       // paged results (k > 64)
    WaveTopK wtk;
    wtk.init(k);
    for (int j = y; j < np; j += split) {
        const uint32_t p = probes[q * np + j];
        const int64_t R0 = part_off[p], R1 = part_off[p + 1];
        const int64_t tt0 = R0 >> 6, tt1 = (R1 + 63) >> 6;
        for (int64_t b0 = tt0; b0 < tt1; b0 += static_cast<int64_t>(kAdcWaves) * kWideTiles) {
            bool want[kWideTiles], live[kWideTiles];
            float total[kWideTiles];
#pragma unroll
            for (int tb = 0; tb < kWideTiles; tb++) {
                const int64_t tile = b0 + static_cast<int64_t>(tb) * kAdcWaves + wave;
                const int64_t row = tile * 64 + lane;
                live[tb] = tile < tt1 && row >= R0 && row < R1 && row < n_rows && mask_bit(mq, row);
                want[tb] = __any(live[tb]) != 0;
            }
            adc_wide_walk<kAdcWaves>(tiles, groups, m, image, lut, b0, want, tid, total);
#pragma unroll
            for (int tb = 0; tb < kWideTiles; tb++) {
                if (!want[tb]) continue;
                const int64_t row = (b0 + static_cast<int64_t>(tb) * kAdcWaves + wave) * 64 + lane;
                uint64_t key = live[tb] ? make_key(total[tb], static_cast<uint32_t>(row), desc) : kKeyMax;
                if (min_keys && key <= floor_key) key = kKeyMax;
                wtk.offer(key, lane);
            }
        }
    }
    __syncthreads();
    wg_rank_merge<kAdcWaves>(wtk, buf, reinterpret_cast<int *>(buf + kAdcWaves * 64), wave, lane, tid, k,
                             partial + (q * split + y) * k);
}

static int32_t launch_scan_wide(const vg_index *idx, const float *tables, int64_t nq, int k, int slices,
                                uint64_t *partial, hipStream_t st)
{
    const size_t lds = kWideLdsBytes;
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pq_adc_scan_wide_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    const int64_t max_q = (1ll << 30) / slices;
    for (int64_t q0 = 0; q0 < nq; q0 += max_q) {
        const int64_t cnt = nq - q0 < max_q ? nq - q0 : max_q;
        ProfScope prof(idx->ctx, "pq_adc_scan", st);
        VG_LAUNCH(pq_adc_scan_wide_kernel, dim3(static_cast<unsigned>(cnt * slices)), dim3(kAdcThreads), lds, st,
                  reinterpret_cast<const uint4 *>(idx->d_pq_tiles), idx->n, idx->n_tiles, idx->pq->m, idx->pq_groups,
                  tables + q0 * lut_image_words(idx->pq->m), slices, static_cast<int>(cnt), k, partial + q0 * slices * k);
    }
    return VG_OK;
}

static int32_t launch_probe_scan_adc_wide(const vg_index *idx, const float *tables, const uint32_t *probes, const uint32_t *part_off,
                                          int64_t nq, int np, int split, int k, uint64_t *partial, const uint64_t *min_keys, bool desc,
                                          const uint8_t *mask, int64_t mask_stride, hipStream_t st)
{
    const vg_pq *pq = idx->pq;
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pq_adc_probe_wide_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(kWideLdsBytes)));
    for (int64_t q0 = 0; q0 < nq; q0 += 65535) {
        const int64_t cnt = nq - q0 < 65535 ? nq - q0 : 65535;
        ProfScope prof(idx->ctx, "pq_adc_probe", st);
        VG_LAUNCH(pq_adc_probe_wide_kernel, dim3(static_cast<unsigned>(split), static_cast<unsigned>(cnt)), dim3(kAdcThreads),
                  kWideLdsBytes, st, reinterpret_cast<const uint4 *>(idx->d_pq_tiles), idx->n, pq->m, idx->pq_groups,
                  tables + q0 * lut_image_words(pq->m), probes + q0 * np, part_off, np, split, k, partial + q0 * split * k,
                  min_keys ? min_keys + q0 : nullptr, desc, mask ? mask + q0 * mask_stride : nullptr, mask_stride);
    }
    return VG_OK;
}

}  // namespace vg

VG_API int32_t vg_index_set_pq_codes(vg_index *idx, vg_pq *pq, const uint8_t *codes, void *stream)
{
    VG_CHECK(idx && pq, VG_ERR_INVALID_ARG, "vg_index_set_pq_codes: NULL handle");
    VG_CHECK(pq->trained, VG_ERR_NOT_TRAINED, "ProductQuantizer not trained");
    VG_CHECK(pq->dim == idx->dim, VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
    VG_CHECK(idx->n == 0 || codes, VG_ERR_INVALID_ARG, "vg_index_set_pq_codes: codes is NULL");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    if (idx->d_pq_tiles) {
        VG_HIP(hipStreamSynchronize(st));
        VG_HIP(hipFree(idx->d_pq_tiles));
        idx->d_pq_tiles = nullptr;
    }
    VG_TRY(vg::nom_free(idx->pq_nom, st));  // the old codes' nomination (vg_index_enable_pq_nomination / _from_codes again after new codes)
    idx->pq = pq;
    idx->pq_groups = (pq->m + 15) / 16;
    idx->n_tiles = (idx->n + 63) / 64;
    if (idx->n == 0) return VG_OK;
    size_t bytes = static_cast<size_t>(idx->n_tiles) * idx->pq_groups * 64 * 16;
    VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_pq_tiles), bytes));
    vg::DevIn<uint8_t> in;
    VG_TRY(in.init(codes, static_cast<size_t>(idx->n) * pq->m, st));
    // row-major copy for random access by node id (Vamana search)
    if (idx->d_pq_rows) {
        VG_HIP(hipFree(idx->d_pq_rows));
        idx->d_pq_rows = nullptr;
    }
    VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_pq_rows), static_cast<size_t>(idx->n) * pq->m));
    VG_HIP(hipMemcpyAsync(idx->d_pq_rows, in.ptr, static_cast<size_t>(idx->n) * pq->m, hipMemcpyDeviceToDevice, st));
    int64_t total = idx->n_tiles * idx->pq_groups * 64;
    VG_LAUNCH(vg::pq_retile_kernel, dim3(static_cast<unsigned>((total + 255) / 256)),
                       dim3(256), 0, st, in.ptr, idx->n, pq->m, idx->pq_groups, idx->n_tiles,
                       reinterpret_cast<uint4 *>(idx->d_pq_tiles));
    VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}

VG_API int32_t vg_search_pq_adc(vg_index *idx, const float *queries, int64_t nq, int32_t k,
                                uint32_t *ids, float *scores, void *stream)
{
    return vg::pq_adc_search_masked(idx, queries, nq, k, nullptr, 0, false, ids, scores, stream);
}

// vg_search_pq_adc, and — with `mask` (a DEVICE pointer, bit per row, query q's at mask + q * mask_stride) — the whole-segment
// PQ leg of vg_search_flat_filtered (k_probe.hip; k <= 64 and a table that fits LDS, `desc` by the segment's metric)
namespace vg {
// vg_cand_replay.hpp's scorer for the PQ table scan: pq.AdcDistance of a row's code (flat/segment.go:678-689) — the table's entries
// (BuildDistanceTable, pq.go:468-491: five separately rounded operations per dimension) computed where they are used, summed in
// pqAdcLookupAvx512 order; one lane per row of the row-major codes.  At risk: a non-finite query value, scale or offset, or
// magnitudes whose squares could overflow.
struct PqScorer {
    const uint8_t *codes;     // n * m
    const int8_t *codebooks;  // m * 256 * sd
    const float *scales, *offsets;
    int m, sd;
    __device__ bool risk(int64_t, const float *q, int tid) const
    {
        __shared__ int flag;
        __shared__ float vmax;
        if (tid == 0) vmax = 0.0f;
        __syncthreads();
        bool bad = false;
        float b = 0.0f;
        for (int j = tid; j < m; j += kReplayThreads) {
            bad = bad || !is_finite_f32(scales[j]) || !is_finite_f32(offsets[j]);
            b = fmaxf(b, 128.0f * fabsf(scales[j]) + fabsf(offsets[j]));  // |centroid value| <= 128 |scale| + |offset|
        }
        for (int off = 32; off > 0; off >>= 1) b = fmaxf(b, __shfl_xor(b, off));
        if ((tid & 63) == 0) atomicMax(reinterpret_cast<int *>(&vmax), __float_as_int(b));  // non-negative floats order like their bits
        __syncthreads();
        const float vm = vmax;
        for (int j = tid; j < m * sd; j += kReplayThreads)
            bad = bad || !is_finite_f32(q[j]) || !(score_bound(fabsf(q[j]), vm, false) * static_cast<float>(m * sd) < 1e38f);
        return block_any(bad, &flag, tid);
    }
    __device__ void prepare(int64_t, const float *, int) const {}
    __device__ float entry(const float *q, int j, int c) const
    {
        const int8_t *cb = codebooks + (static_cast<int64_t>(j) * 256 + c) * sd;
        const float scale = scales[j], offset = offsets[j];
        const float *qs = q + j * sd;
        float sum = 0.0f;
        for (int i = 0; i < sd; i++) {
            float v = static_cast<float>(cb[i]) * scale;
            v = v + offset;
            const float d = qs[i] - v;
            const float dd = d * d;
            sum = sum + dd;
        }
        return sum;
    }
    __device__ void score_chunk(int64_t, const float *q, int64_t row0, int64_t n, int tid, float *out) const
    {
        const int64_t row = row0 + tid;
        if (row >= n) return;
        const uint8_t *code = codes + row * m;
        float s[16];
#pragma unroll
        for (int l = 0; l < 16; l++) s[l] = 0.0f;
        int i = 0;
        for (; i + 16 <= m; i += 16)
#pragma unroll
            for (int l = 0; l < 16; l++) s[l] = s[l] + entry(q, i + l, code[i + l]);
        float total = reduce16_regs(s);
        for (; i < m; i++) total = total + entry(q, i, code[i]);
        out[tid] = total;
    }
};
}  // namespace vg

namespace vg {
// the replay for device buffers: the whole segment, or (probes: nq * np partition ids, part_off) the probed partitions; mask: a
// device row filter per query / for the batch, or null; desc: a Dot / Cosine segment keeps the LARGEST sums (flat/segment.go:449)
int32_t pq_nan_replay(vg_index *idx, const float *d_queries, int64_t nq, int k, bool desc, const uint8_t *d_mask, int64_t mask_stride,
                      const uint32_t *d_probes, int np, const uint32_t *d_part_off, uint32_t *d_ids, float *d_scores, hipStream_t st)
{
    if (idx->n == 0) return VG_OK;
    const vg_pq *pq = idx->pq;
    return launch_cand_replay(PqScorer{idx->d_pq_rows, pq->d_codebooks, pq->d_scales, pq->d_offsets, pq->m, pq->subdim}, d_queries, idx->dim, idx->n, nq,
                              k, desc, d_mask, mask_stride, d_ids, d_scores, st, nullptr, d_probes, np, d_part_off);
}
}  // namespace vg

static int32_t pq_adc_search_impl(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask, int64_t mask_stride,
                                  bool desc, uint32_t *ids, float *scores, void *stream, bool allow_nomination);
int32_t vg::pq_adc_search_masked(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask,
                                 int64_t mask_stride, bool desc, uint32_t *ids, float *scores, void *stream)
{
    return pq_adc_search_impl(idx, queries, nq, k, mask, mask_stride, desc, ids, scores, stream, true);
}
static int32_t pq_adc_search_impl(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask, int64_t mask_stride,
                                  bool desc, uint32_t *ids, float *scores, void *stream, bool allow_nomination)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_search_pq_adc: NULL index");
    VG_CHECK(idx->pq != nullptr, VG_ERR_NOT_READY, "vg_search_pq_adc: index has no PQ codes");
    const vg_pq *pq = idx->pq;
    VG_CHECK(pq->trained, VG_ERR_NOT_TRAINED, "ProductQuantizer not trained");
    VG_CHECK(nq >= 0 && k >= 0, VG_ERR_INVALID_ARG, "vg_search_pq_adc: negative nq or k");
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(queries && ids && scores, VG_ERR_INVALID_ARG, "vg_search_pq_adc: NULL buffer");
    VG_CHECK(k <= vg::kAdcMaxK, VG_ERR_UNSUPPORTED, "vg_search_pq_adc: k=%d exceeds %d", k,
             vg::kAdcMaxK);
    // The reference builds the table with stride K and looks it up with stride 256
    // (pq.go:474 vs internal/simd/kernels.go:249); only K == 256 is self-consistent.
    VG_CHECK(pq->k == 256, VG_ERR_UNSUPPORTED,
             "vg_search_pq_adc: LUT scan needs numCentroids == 256 (got %d)", pq->k);
    size_t lds = static_cast<size_t>(vg::lut_image_words(pq->m)) * 4 + vg::kAdcBuf * 8 + sizeof(vg::AdcShared);
    // a table beyond one LDS image (m > 96 at fp32) is walked in 96 KiB chunks: pq_adc_scan_wide_kernel, k <= 64
    const bool wide = lds > 160 * 1024;
    VG_CHECK(mask == nullptr || (!wide && k <= 64), VG_ERR_UNSUPPORTED, "pq_adc_search_masked: k=%d / m=%d take the probe kernels", k, pq->m);
    VG_CHECK(!wide || k <= 64, VG_ERR_UNSUPPORTED,
             "vg_search_pq_adc: m=%d lookup table does not fit the 160 KiB LDS; the chunked scan takes k <= 64", pq->m);
    vg::SearchIO io;
    VG_TRY(io.init(idx->ctx, stream, queries, static_cast<size_t>(nq) * idx->dim, ids, scores, static_cast<size_t>(nq) * k));
    const hipStream_t st = io.st;
    const float *q = io.q.ptr;
    uint32_t *oid = io.oid.ptr;
    float *osc = io.osc.ptr;

    if (idx->n == 0) {
        VG_TRY(vg::empty_results(nq, k, false, oid, osc, st));
    } else if (allow_nomination && vg::pq_nomination_applies(idx, q, nq, k, mask, desc)) {
        std::vector<int> failed;
        VG_TRY(vg::pq_nominated_pass(idx, q, nq, k, oid, osc, st, failed));
        // the table scan for the queries whose proof failed (ties at the k-th score, thresholds too tight)
        VG_TRY(vg::rescan_failed(failed, q, idx->dim, k, nullptr, 0, 0, oid, osc, st,
                                 [&](const float *fq, int64_t nf, const uint8_t *, int64_t, uint32_t *fid, float *fsc) {
                                     return pq_adc_search_impl(idx, fq, nf, k, nullptr, 0, false, fid, fsc, st, false);
                                 }));
    } else {
        // one workgroup per CU: the smallest multiple of 8 (one group per XCD) with slices * nq >= #CUs, at least one
        // workgroup-iteration of tiles (kAdcWaves of them) per slice
        const int64_t tile_groups = (idx->n_tiles + vg::kAdcWaves - 1) / vg::kAdcWaves;
        int slices = vg::scan_slices(nq, tile_groups, idx->ctx->compute_units, 1);
        const bool bigk = k > 64;
        const bool bigk_fast = bigk && !vg::hook(vg::kHookAdcBigkExhaustive);  // test hook: LDS-buffer path only
        // enough waves that a wave expects <= ~8 of the k best rows (capacity 64 each): k / 64 workgroups by the same rule
        if (bigk_fast) slices = std::max(slices, vg::scan_slices(1, tile_groups, k / 64, 1));
        vg::ArenaCall ar(idx->ctx, st);
        const int i_tables = ar.add(sizeof(float) * static_cast<size_t>(nq) * vg::lut_image_words(pq->m));
        const int i_partial = ar.add(sizeof(uint64_t) * static_cast<size_t>(nq) * slices *
                                     (bigk_fast ? std::max(k, vg::kAdcWaves * 64) : k));
        const int i_flags = ar.add(bigk_fast ? sizeof(int) * static_cast<size_t>(nq) : 0);
        const int i_fid = ar.add(bigk_fast ? sizeof(uint32_t) * static_cast<size_t>(nq) * k : 0);
        const int i_fsc = ar.add(bigk_fast ? sizeof(float) * static_cast<size_t>(nq) * k : 0);
        VG_TRY(ar.commit());
        float *tables = ar.get<float>(i_tables);
        uint64_t *partial = ar.get<uint64_t>(i_partial);
        VG_TRY(vg::launch_pq_build_table(pq, q, nq, tables, true, st));
        if (bigk_fast) {
            int *flags = ar.get<int>(i_flags);
            uint32_t *fid = ar.get<uint32_t>(i_fid);
            float *fsc = ar.get<float>(i_fsc);
            // (1) every wave keeps its 64 best; (2) select k of the union and prove it; (3) the
            // exhaustive LDS-buffer scan re-runs only for queries whose proof failed
            if (pq->m == 96)
                VG_TRY((vg::launch_scan<6, true>(idx, tables, nq, k, slices, partial, st, 1)));
            else
                VG_TRY((vg::launch_scan<-1, true>(idx, tables, nq, k, slices, partial, st, 1)));
            VG_LAUNCH(vg::topk_select_verify_kernel, dim3(static_cast<unsigned>(nq)), dim3(vg::kMergeThreads), 0, st,
                      partial, slices * vg::kAdcWaves, k, false, oid, osc, flags);
            if (pq->m == 96)
                VG_TRY((vg::launch_scan<6, false>(idx, tables, nq, k, slices, partial, st, 0, flags)));
            else
                VG_TRY((vg::launch_scan<-1, false>(idx, tables, nq, k, slices, partial, st, 0, flags)));
            VG_TRY(vg::launch_topk_merge(partial, nq, slices, k, false, fid, fsc, st, flags));
            VG_LAUNCH(vg::patch_results_kernel, dim3(static_cast<unsigned>(nq)), dim3(64), 0, st, flags, k, fid, fsc,
                      oid, osc);
        } else {
            if (wide)
                VG_TRY(vg::launch_scan_wide(idx, tables, nq, k, slices, partial, st));
            else if (pq->m == 96 && k <= 64)
                VG_TRY((vg::launch_scan<6, true>(idx, tables, nq, k, slices, partial, st, 0, nullptr, mask, mask_stride, desc)));
            else if (pq->m == 96)
                VG_TRY((vg::launch_scan<6, false>(idx, tables, nq, k, slices, partial, st)));
            else if (k <= 64)
                VG_TRY((vg::launch_scan<-1, true>(idx, tables, nq, k, slices, partial, st, 0, nullptr, mask, mask_stride, desc)));
            else
                VG_TRY((vg::launch_scan<-1, false>(idx, tables, nq, k, slices, partial, st)));
            VG_TRY(vg::launch_topk_merge(partial, nq, slices, k, desc, oid, osc, st));
        }
    }
    // queries whose table sums may hold a NaN: the reference's heap, operation by operation (vg_cand_replay.hpp; not for the queries
    // this function sends to itself after a failed proof: the caller's pass covers them)
    if (allow_nomination) VG_TRY(vg::pq_nan_replay(idx, q, nq, k, desc, mask, mask_stride, nullptr, 0, nullptr, oid, osc, st));
    return io.finish();
}
