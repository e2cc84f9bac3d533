// k_probed_threshold.hip — Engine.SearchThreshold (engine/engine.go:1485-1531) over a flat segment with codes and / or IVF
// partitions: flat.Segment.Search(q, k = max_results, nprobes, filter) with the segment's scan (flat/segment.go:447-751: fp32
// rows, SQ8 codes, PQ table lookups; the whole segment or the nprobes closest partitions), Segment.Rerank (:754-780) and the
// engine's filter (:1518-1529).
//   One scan kernel family, templated on the row scorer, walks the rows a query can see — the whole segment in pieces, up to 8
//   queries per pass over the rows, or one (query, probe) pair's partition — and bounds what it keeps in one of two ways:
//   (a) the user's threshold fused: a row is appended to its query's list iff its scan score passes (the list holds every row the
//       query can see: it cannot overflow); flat_thr_select_kernel then keeps the best max_results.  rerank == 0, and fp32 rows
//       either way (their scan score IS the exact score).
//   (b) the best max_results rows by CODE score (rerank != 0 over SQ8 / PQ, where the threshold says nothing about code scores):
//       pass 1 histograms the top 16 bits of every visible row's key into 65536 bins per query, a small kernel finds the first
//       bin at which the running count reaches max_results, pass 2 appends every key at or below that bin, the selection keeps the
//       best max_results.  Ties and clustered scores make the list longer, never wrong: no proof, no fallback.  Then the selected
//       rows are re-scored exactly against the user's threshold (flat_thr_rescore_kernel) and selected again.
//   A query whose scan scores may hold a NaN has its candidate stage replayed through the reference's heap at k = max_results
//   (vg_cand_replay.hpp) before the rerank / filter.
#include <algorithm>
#include <functional>
#include <vector>

#include "vg_adc_row.hpp"
#include "vg_adc_wide.hpp"
#include "vg_cand_replay.hpp"
#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"
#include "vg_sq8_row.hpp"

namespace vg {

constexpr int kPthrBins = 65536;        // the top 16 bits of a key
constexpr size_t kPthrLutMax = 96 * 1024;  // a PQ table image the scan holds in LDS (m <= 96 at 256 centroids); beyond: pthr_scan_wide_kernel
enum PthrMode { kPthrThr = 0, kPthrHist = 1, kPthrBin = 2 };

// the query of slot s of a launch (qmap null: s)
__device__ __forceinline__ int64_t pthr_query(const int *__restrict__ qmap, int64_t s) { return qmap ? qmap[s] : s; }

// ---- the row scorers ----------------------------------------------------------------------------------------------------
// kRows rows per wave step, row_of(lane) the lane's row within the step, owner(lane) the lane that reports it.  prepare() once per
// workgroup (queries: the launch's; the pass is slots q0 .. q0 + cnt - 1; LDS staging), begin_row() per step, score() per (step,
// slot qi of the pass, q its query) by ALL lanes of the wave.  Scores are bit for bit vg_search_flat_probed's for the same row.

// fp32 rows, 16 lanes per row (flat/segment.go:691-701).  REGS: the row once into registers, the queries in LDS
// (exact_rowregs16: dim % 4 == 0, 64 <= dim <= 1024, 16-byte aligned rows); else every pair from memory (exact_pair16, any dim)
template <bool DOT, bool REGS>
struct PthrF32 {
    static constexpr int kRows = 4;
    static constexpr bool desc = DOT;
    const float *base;
    int dim;
    struct Row {
        Sub16 sub;
        const float *row;
        float4 rr[16];
    };
    __device__ static int row_of(int lane) { return lane >> 4; }
    __device__ static bool owner(int lane) { return (lane & 15) == 0; }
    __device__ void prepare(Row &r, float *lds, const float *queries, const int *qmap, int64_t q0, int cnt, int tid) const
    {
        r.sub = Sub16::make(tid);
        if (REGS) {
            for (int t = tid; t < cnt * dim; t += 256) {
                const int qi = t / dim;
                lds[t] = queries[pthr_query(qmap, q0 + qi) * dim + (t - qi * dim)];
            }
            __syncthreads();
        }
    }
    // row: clamped by the caller to a row of the index
    __device__ void begin_row(Row &r, int64_t row, int) const
    {
        r.row = base + row * dim;
        if (REGS) {
            const float4 *r4 = reinterpret_cast<const float4 *>(r.row) + r.sub.f4;
            const int nblk = dim >> 6;
#pragma unroll
            for (int e = 0; e < 16; e++)
                if (e < nblk) r.rr[e] = load_stream(r4 + e * 16);  // (a pass reads a row once)
        }
    }
    __device__ float score(const Row &r, const float *lds, const float *q, int qi) const
    {
        return REGS ? exact_rowregs16<DOT>(r.rr, dim >> 6, r.row, lds + static_cast<size_t>(qi) * dim, dim, r.sub)
                    : exact_pair16<DOT, kPair>(r.row, q, dim, r.sub);
    }
};

// SQ8 codes, one lane per row of a 64-row tile (flat/segment.go:517-604, :659-667)
template <bool DOT>
struct PthrSq8 {
    static constexpr int kRows = 64;
    static constexpr bool desc = DOT;
    const uint4 *tiles;
    const float *mins, *inv;
    int groups, dim;
    struct Row {
        const uint4 *tp;
    };
    __device__ static int row_of(int lane) { return lane; }
    __device__ static bool owner(int) { return true; }
    __device__ void prepare(Row &, float *, const float *, const int *, int64_t, int, int) const {}
    __device__ void begin_row(Row &r, int64_t row, int lane) const { r.tp = tiles + ((row >> 6) * groups) * 64 + lane; }
    __device__ float score(const Row &r, const float *, const float *q, int) const
    {
        return sq8_row_score<DOT>(r.tp, groups, dim >> 4, dim & 15, q, mins, inv);
    }
};

// PQ codes, one lane per row; the query's BuildDistanceTable image (the scan layout of k_adc.hip) in LDS, one query per pass
struct PthrPq {
    static constexpr int kRows = 64;
    const uint4 *tiles;
    const float *tables;  // per slot of the launch: lut_image_words(m)
    int m, groups;
    bool desc;
    struct Row {
        const uint4 *tp;
        int rot;
    };
    __device__ static int row_of(int lane) { return lane; }
    __device__ static bool owner(int) { return true; }
    __device__ void prepare(Row &, float *lds, const float *, const int *, int64_t q0, int, int tid) const
    {
        const int n4 = lut_image_words(m) / 4;
        const float4 *src = reinterpret_cast<const float4 *>(tables + q0 * lut_image_words(m));
        float4 *dst = reinterpret_cast<float4 *>(lds);
        for (int i = tid; i < n4; i += 256) dst[i] = src[i];
        __syncthreads();
    }
    __device__ void begin_row(Row &r, int64_t row, int lane) const
    {
        r.tp = tiles + ((row >> 6) * groups) * 64 + lane;
        r.rot = lane & 15;
    }
    __device__ float score(const Row &r, const float *lds, const float *, int) const { return adc_row_score_lds(lds, r.tp, m, r.rot); }
};

// Pass 1's counts go through a small histogram in LDS first: a query's scores cluster — 128 bins per octave — so every wave of
// the device would otherwise add into the same few dozen words of HBM.  kPthrSlots direct-mapped slots per query of the pass,
// slot = bin % kPthrSlots, tagged with the bin that took it: a run of up to kPthrSlots consecutive bins (8 octaves) maps without
// collisions; a bin that finds its slot taken by another goes to the HBM histogram directly.  The workgroup adds its slots to HBM
// at the end.
constexpr int kPthrSlots = 1024;
constexpr uint32_t kPthrNoBin = 0xFFFFFFFFu;
// the lanes with `on` add one to their bin: one LDS operation per distinct bin of the wave
__device__ __forceinline__ void wave_hist(bool on, uint32_t bin, uint32_t *tags, unsigned *slots, unsigned *hist, int lane)
{
    uint64_t m = __ballot(on);
    while (m != 0) {
        const int first = __builtin_ctzll(m);
        const uint32_t b = __shfl(bin, first);
        const uint64_t same = __ballot(on && bin == b);
        if (lane == first) {
            const unsigned add = static_cast<unsigned>(__popcll(same));
            const uint32_t slot = b & (kPthrSlots - 1);
            const uint32_t old = atomicCAS(&tags[slot], kPthrNoBin, b);
            if (old == kPthrNoBin || old == b)
                atomicAdd(&slots[slot], add);
            else
                atomicAdd(&hist[b], add);
        }
        m &= ~same;
    }
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
// grid (slice, range j, pass): pass g carries slots g * QB .. of the launch's nq.  Slot s answers query q = qmap[s] (null: s — the
// queries a failed proof sends back to vg_search_flat_threshold are scattered): it reads q's row of queries, thr and mask, and
// writes list, count, histogram and cut s.  probes (QB == 1, no qmap): range j is partition
// probes[s * np + j], rows part_off[p] .. part_off[p + 1] — it may start anywhere inside a wave step, an empty partition is two
// equal offsets; null: piece j of np equal pieces of the whole segment.  A range is walked in steps of S::kRows rows aligned to
// kRows (the SQ8 / PQ tiles), the rows outside it masked.  mask: bit i of byte i / 8 of query q's filter at
// mask + q * mask_stride (stride 0: one filter), or null.
// MODE kPthrThr: a row whose score passes thr[q] is appended to lists[s]; kPthrHist: bin (key >> 48) of hist[s] counts it;
// kPthrBin: appended when its bin is at or below cut[s].
template <class S, int MODE, int QB>
__global__ __launch_bounds__(256) void pthr_scan_kernel(const S sc, const float *__restrict__ queries, const int *__restrict__ qmap, int dim,
                                                        int64_t nq, int64_t n, const uint32_t *__restrict__ probes,
                                                        const uint32_t *__restrict__ part_off, int np, int sub_n, const float *__restrict__ thr,
                                                        const uint32_t *__restrict__ cut, const uint8_t *__restrict__ mask,
                                                        int64_t mask_stride, int64_t list_cap, uint64_t *__restrict__ lists,
                                                        int *__restrict__ counts, unsigned *__restrict__ hist, int scorer_lds_words)
{
    extern __shared__ __attribute__((aligned(16))) float pthr_lds[];  // the scorer's; kPthrHist: then QB * kPthrSlots tags and counts
    const int s = blockIdx.x, j = blockIdx.y;
    const int64_t q0 = static_cast<int64_t>(blockIdx.z) * QB;
    const int cnt = static_cast<int>(nq - q0 < QB ? nq - q0 : QB);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t R0, R1;
    if (probes) {
        const uint32_t p = probes[q0 * np + j];
        R0 = part_off[p];
        R1 = part_off[p + 1];
    } else {
        R0 = n * j / np;
        R1 = n * (j + 1) / np;
    }
    if (R1 <= R0) return;  // (the whole workgroup)
    typename S::Row rs;
    sc.prepare(rs, pthr_lds, queries, qmap, q0, cnt, tid);
    float tq[QB];
    uint32_t cq[QB];
    const uint8_t *mq[QB];
    const float *qv[QB];
#pragma unroll
    for (int qi = 0; qi < QB; qi++) {
        const int64_t slot = qi < cnt ? q0 + qi : q0, qq = pthr_query(qmap, slot);
        tq[qi] = MODE == kPthrThr ? thr[qq] : 0.0f;
        cq[qi] = MODE == kPthrBin ? cut[slot] : 0u;
        mq[qi] = mask ? mask + qq * mask_stride : nullptr;
        qv[qi] = queries + qq * dim;
    }
    uint32_t *htags = reinterpret_cast<uint32_t *>(pthr_lds + scorer_lds_words);
    unsigned *hslots = htags + QB * kPthrSlots;
    if (MODE == kPthrHist) {
        for (int t = tid; t < QB * kPthrSlots; t += 256) {
            htags[t] = kPthrNoBin;
            hslots[t] = 0u;
        }
        __syncthreads();
    }
    const int64_t u0 = R0 / S::kRows, u1 = (R1 + S::kRows - 1) / S::kRows;
    const int64_t t0 = u0 + (u1 - u0) * s / sub_n, t1 = u0 + (u1 - u0) * (s + 1) / sub_n;
    for (int64_t u = t0 + wave; u < t1; u += 4) {
        const int64_t row = u * S::kRows + S::row_of(lane);
        const bool in = row >= R0 && row < R1;
        bool want = in;  // some query of the pass takes the row (filter.Matches)
        if (mask) {
            want = false;
#pragma unroll
            for (int qi = 0; qi < QB; qi++) want = want || (in && qi < cnt && mask_bit(mq[qi], row));
        }
        if (!__any(want)) continue;  // a step the range or the filter leaves nothing of: its rows are not read
        sc.begin_row(rs, in ? row : (row < R0 ? R0 : R1 - 1), lane);
#pragma unroll
        for (int qi = 0; qi < QB; qi++) {
            if (qi < cnt) {
                const float v = sc.score(rs, pthr_lds, qv[qi], qi);
                const uint64_t key = make_key(v, static_cast<uint32_t>(row), sc.desc);
                const bool live = in && S::owner(lane) && mask_bit(mq[qi], in ? row : R0);
                const uint32_t bin = static_cast<uint32_t>(key >> 48);
                if (MODE == kPthrHist) {
                    wave_hist(live, bin, htags + qi * kPthrSlots, hslots + qi * kPthrSlots, hist + (q0 + qi) * kPthrBins, lane);
                } else {
                    const bool pass = live && (MODE == kPthrBin ? bin <= cq[qi] : (sc.desc ? v >= tq[qi] : v <= tq[qi]));
                    wave_append(pass, key, counts + q0 + qi, lists + (q0 + qi) * list_cap, lane);
                }
            }
        }
    }
    if (MODE == kPthrHist) {
        __syncthreads();
        for (int t = tid; t < cnt * kPthrSlots; t += 256)
            if (hslots[t] != 0u) atomicAdd(&hist[(q0 + t / kPthrSlots) * kPthrBins + htags[t]], hslots[t]);
    }
}

// the first bin at which a query's running count reaches max_results (every bin when the query sees fewer rows)
__global__ __launch_bounds__(1024) void pthr_cut_kernel(const unsigned *__restrict__ hist, int max_results, uint32_t *__restrict__ cut)
{
    __shared__ unsigned part[1024];
    const int tid = threadIdx.x;
    const unsigned *h = hist + static_cast<int64_t>(blockIdx.x) * kPthrBins + tid * (kPthrBins / 1024);
    unsigned sum = 0;
    for (int i = 0; i < kPthrBins / 1024; i++) sum += h[i];
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned v = tid >= off ? part[tid - off] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const unsigned want = static_cast<unsigned>(max_results), incl = part[tid], excl = incl - sum;
    if (tid == 0 && part[1023] < want) cut[blockIdx.x] = kPthrBins - 1;
    if (excl < want && incl >= want) {
        unsigned run = excl;
        for (int i = 0; i < kPthrBins / 1024; i++) {
            run += h[i];
            if (run >= want) {
                cut[blockIdx.x] = static_cast<uint32_t>(tid * (kPthrBins / 1024) + i);
                break;
            }
        }
    }
}

struct PthrArgs {
    const float *queries;
    const int *qmap;
    int dim;
    int64_t nq, n;
    const uint32_t *probes, *part_off;
    int np, sub;
    const float *thr;
    const uint32_t *cut;
    const uint8_t *mask;
    int64_t mask_stride, list_cap;
    uint64_t *lists;
    int *counts;
    unsigned *hist;
};

template <class S, int QB>
static int32_t launch_pthr(const S &sc, int mode, size_t lds, const PthrArgs &a, hipStream_t st)
{
    const dim3 grid(static_cast<unsigned>(a.sub), static_cast<unsigned>(a.np), static_cast<unsigned>((a.nq + QB - 1) / QB));
    const size_t bytes = lds + (mode == kPthrHist ? sizeof(uint32_t) * 2 * QB * kPthrSlots : 0);
    auto go = [&](auto kern) -> int32_t {
        if (bytes > 48 * 1024)
            VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
        VG_LAUNCH(kern, grid, dim3(256), bytes, st, sc, a.queries, a.qmap, a.dim, a.nq, a.n, a.probes, a.part_off, a.np, a.sub, a.thr, a.cut,
                  a.mask, a.mask_stride, a.list_cap, a.lists, a.counts, a.hist, static_cast<int>(lds / sizeof(float)));
        return VG_OK;
    };
    if (mode == kPthrHist) return go(pthr_scan_kernel<S, kPthrHist, QB>);
    if (mode == kPthrBin) return go(pthr_scan_kernel<S, kPthrBin, QB>);
    return go(pthr_scan_kernel<S, kPthrThr, QB>);
}

// ---- the scan over a PQ table beyond one LDS image (m > 96) -----------------------------------------------------------------
// pthr_scan_kernel<PthrPq, MODE, 1>'s sibling: same grid, ranges, slices, mask, slot map and consumers, but the scores of a batch
// of kWideTiles tiles per wave come out of one walk over the table's chunks (adc_wide_walk, vg_adc_wide.hpp) — pthr_scan_kernel
// scores a row step at a time against a whole image, so this is a kernel of its own, not a scorer.  tables: per slot.
// LDS: the walker's chunk and tail rows (111 KiB), kPthrHist: then the histogram slots (8 KiB).  One workgroup per CU, 8 waves.
constexpr int kPthrWideWaves = 8;
template <int MODE>
__global__ __launch_bounds__(kPthrWideWaves * 64) void pthr_scan_wide_kernel(
    const uint4 *__restrict__ tiles, const float *__restrict__ tables, int m, int groups, bool desc, const int *__restrict__ qmap, int64_t n,
    const uint32_t *__restrict__ probes, const uint32_t *__restrict__ part_off, int np, int sub_n, const float *__restrict__ thr,
    const uint32_t *__restrict__ cut, const uint8_t *__restrict__ mask, int64_t mask_stride, int64_t list_cap, uint64_t *__restrict__ lists,
    int *__restrict__ counts, unsigned *__restrict__ hist)
{
    extern __shared__ __attribute__((aligned(16))) float pthr_lds[];
    constexpr int kThreads = kPthrWideWaves * 64;
    const int s = blockIdx.x, j = blockIdx.y;
    const int64_t slot = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t R0, R1;
    if (probes) {
        const uint32_t p = probes[slot * np + j];
        R0 = part_off[p];
        R1 = part_off[p + 1];
    } else {
        R0 = n * j / np;
        R1 = n * (j + 1) / np;
    }
    if (R1 <= R0) return;  // (the whole workgroup)
    const int64_t qq = pthr_query(qmap, slot);
    const float tq = MODE == kPthrThr ? thr[qq] : 0.0f;
    const uint32_t cq = MODE == kPthrBin ? cut[slot] : 0u;
    const uint8_t *mq = mask ? mask + qq * mask_stride : nullptr;
    const float *image = tables + slot * lut_image_words(m);
    uint32_t *htags = reinterpret_cast<uint32_t *>(pthr_lds + kWideLdsWords);
    unsigned *hslots = htags + kPthrSlots;
    if (MODE == kPthrHist) {
        for (int t = tid; t < kPthrSlots; t += kThreads) {
            htags[t] = kPthrNoBin;
            hslots[t] = 0u;
        }
        __syncthreads();
    }
    const int64_t u0 = R0 >> 6, u1 = (R1 + 63) >> 6;
    const int64_t t0 = u0 + (u1 - u0) * s / sub_n, t1 = u0 + (u1 - u0) * (s + 1) / sub_n;
    for (int64_t b0 = t0; b0 < t1; b0 += static_cast<int64_t>(kPthrWideWaves) * kWideTiles) {
        bool want[kWideTiles], live[kWideTiles];
        float total[kWideTiles];
#pragma unroll
        for (int tb = 0; tb < kWideTiles; tb++) {
            const int64_t tile = b0 + static_cast<int64_t>(tb) * kPthrWideWaves + wave;
            const int64_t row = tile * 64 + lane;
            live[tb] = tile < t1 && row >= R0 && row < R1 && mask_bit(mq, row);  // (filter.Matches)
            want[tb] = __any(live[tb]) != 0;  // a tile the range or the filter leaves nothing of: its rows are not read
        }
        adc_wide_walk<kPthrWideWaves>(tiles, groups, m, image, pthr_lds, b0, want, tid, total);
#pragma unroll
        for (int tb = 0; tb < kWideTiles; tb++) {
            if (!want[tb]) continue;
            const int64_t row = (b0 + static_cast<int64_t>(tb) * kPthrWideWaves + wave) * 64 + lane;
            const float v = total[tb];
            const uint64_t key = make_key(v, static_cast<uint32_t>(row), desc);
            const uint32_t bin = static_cast<uint32_t>(key >> 48);
            if (MODE == kPthrHist) {
                wave_hist(live[tb], bin, htags, hslots, hist + slot * kPthrBins, lane);
            } else {
                const bool pass = live[tb] && (MODE == kPthrBin ? bin <= cq : (desc ? v >= tq : v <= tq));
                wave_append(pass, key, counts + slot, lists + slot * list_cap, lane);
            }
        }
    }
    if (MODE == kPthrHist) {
        __syncthreads();
        for (int t = tid; t < kPthrSlots; t += kThreads)
            if (hslots[t] != 0u) atomicAdd(&hist[slot * kPthrBins + htags[t]], hslots[t]);
    }
}

static int32_t launch_pthr_wide(const vg_index *idx, const float *tables, bool desc, int mode, const PthrArgs &a, hipStream_t st)
{
    const dim3 grid(static_cast<unsigned>(a.sub), static_cast<unsigned>(a.np), static_cast<unsigned>(a.nq));
    const size_t bytes = sizeof(float) * kWideLdsWords + (mode == kPthrHist ? sizeof(uint32_t) * 2 * kPthrSlots : 0);
    auto go = [&](auto kern) -> int32_t {
        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
        VG_LAUNCH(kern, grid, dim3(kPthrWideWaves * 64), bytes, st, reinterpret_cast<const uint4 *>(idx->d_pq_tiles), tables, idx->pq->m,
                  idx->pq_groups, desc, a.qmap, a.n, a.probes, a.part_off, a.np, a.sub, a.thr, a.cut, a.mask, a.mask_stride, a.list_cap, a.lists,
                  a.counts, a.hist);
        return VG_OK;
    };
    if (mode == kPthrHist) return go(pthr_scan_wide_kernel<kPthrHist>);
    if (mode == kPthrBin) return go(pthr_scan_wide_kernel<kPthrBin>);
    return go(pthr_scan_wide_kernel<kPthrThr>);
}

// the scorer of the call: scan kind, metric, the fp32 register form; qb: kThrQB (the whole segment, fp32 / SQ8) or 1
static int32_t pthr_pass(const vg_index *idx, int32_t scan, int qb, const float *tables, int mode, const PthrArgs &a, hipStream_t st)
{
    VG_CHECK(!(a.qmap && a.probes), VG_ERR_INVALID_ARG, "pthr_pass: a slot map over probed partitions");
    const bool dot = idx->metric != VG_METRIC_L2;
    if (scan == VG_SCAN_PQ) {
        // a table beyond one LDS image: the chunked sibling (test hook kHookAdcWideAlways: whatever m is)
        if (sizeof(float) * static_cast<size_t>(lut_image_words(idx->pq->m)) > kPthrLutMax || hook(kHookAdcWideAlways))
            return launch_pthr_wide(idx, tables, dot, mode, a, st);
        const PthrPq sc{reinterpret_cast<const uint4 *>(idx->d_pq_tiles), tables, idx->pq->m, idx->pq_groups, dot};
        return launch_pthr<PthrPq, 1>(sc, mode, sizeof(float) * static_cast<size_t>(lut_image_words(idx->pq->m)), a, st);
    }
    auto with_qb = [&](auto sc, size_t lds_per_query) -> int32_t {
        using S = decltype(sc);
        return qb == 1 ? launch_pthr<S, 1>(sc, mode, lds_per_query, a, st) : launch_pthr<S, kThrQB>(sc, mode, lds_per_query * kThrQB, a, st);
    };
    return with_metric(dot, [&](auto dot_c) -> int32_t {
        constexpr bool DOT = decltype(dot_c)::value;
        if (scan == VG_SCAN_SQ8)
            return with_qb(PthrSq8<DOT>{reinterpret_cast<const uint4 *>(idx->d_sq_tiles), idx->sq->d_mins, idx->sq->d_inv, idx->sq_groups,
                                        idx->dim}, 0);
        if (thr_scan_regs(idx)) return with_qb(PthrF32<DOT, true>{idx->d_vectors, idx->dim}, sizeof(float) * static_cast<size_t>(idx->dim));
        return with_qb(PthrF32<DOT, false>{idx->d_vectors, idx->dim}, 0);
    });
}

// the grid of a launch of `slots` slots, qb per pass: the ranges of a pass (np probed partitions; np 0: the whole segment in up to
// 64 pieces of at least 4096 rows) and the slices of a range, for ~4 workgroups per CU (PQ: one, its table fills the LDS)
static void pthr_grid(const vg_index *idx, int32_t scan, int np, int64_t slots, int qb, int &ranges, int &sub)
{
    ranges = np ? np : static_cast<int>(std::min<int64_t>(64, std::max<int64_t>(1, idx->n / 4096)));
    const int64_t passes = (slots + qb - 1) / qb * ranges;
    const int64_t want_wgs = (scan == VG_SCAN_PQ ? 1 : 4) * static_cast<int64_t>(idx->ctx->compute_units);
    sub = static_cast<int>(std::min<int64_t>(32, std::max<int64_t>(1, (want_wgs + passes - 1) / passes)));
}

int32_t launch_thr_scan_f32(const vg_index *idx, const float *queries, const float *thr, const int *qmap, int64_t cnt,
                            const uint8_t *mask, int64_t mask_stride, int64_t list_cap, uint64_t *lists, int *counts, hipStream_t st)
{
    int ranges, sub;
    pthr_grid(idx, VG_SCAN_F32, 0, cnt, kThrQB, ranges, sub);
    const PthrArgs a{queries, qmap, idx->dim, cnt, idx->n, nullptr, nullptr, ranges, sub, thr, nullptr, mask, mask_stride, list_cap, lists,
                     counts, nullptr};
    return pthr_pass(idx, VG_SCAN_F32, kThrQB, nullptr, kPthrThr, a, st);
}

}  // namespace vg

VG_API int32_t vg_search_flat_probed_threshold(vg_index *idx, const float *queries, int64_t nq, const float *thresholds,
                                               int32_t max_results, int32_t nprobes, int32_t scan, int32_t rerank,
                                               const uint8_t *mask, int64_t mask_stride, uint32_t *ids, float *scores,
                                               int32_t *counts, void *stream)
{
    const char *fn = "vg_search_flat_probed_threshold";
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(nq >= 0 && max_results >= 0, VG_ERR_INVALID_ARG, "%s: negative nq or max_results", fn);
    VG_CHECK(scan == VG_SCAN_F32 || scan == VG_SCAN_PQ || scan == VG_SCAN_SQ8, VG_ERR_INVALID_ARG, "%s: unknown scan type %d", fn, scan);
    VG_CHECK(max_results <= vg::kThrMaxResults, VG_ERR_UNSUPPORTED, "%s: max_results=%d exceeds %d", fn, max_results, vg::kThrMaxResults);
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    const bool whole = idx->num_partitions <= 1;  // segment.go:745-749: one range, the whole segment
    int np = nprobes <= 0 ? 1 : nprobes;          // segment.go:728-731
    if (np > idx->num_partitions) np = idx->num_partitions;  // kmeans.go:219-221
    VG_CHECK(whole || np <= 64, VG_ERR_UNSUPPORTED, "%s: nprobes=%d exceeds 64", fn, np);
    const int64_t n = idx->n;
    if (scan == VG_SCAN_F32) {
        VG_CHECK(n == 0 || idx->d_vectors, VG_ERR_NOT_READY, "%s: index has no fp32 vectors", fn);
    } else if (scan == VG_SCAN_PQ) {
        VG_CHECK(idx->pq && (n == 0 || idx->d_pq_tiles), VG_ERR_NOT_READY, "%s: index has no PQ codes", fn);
        VG_CHECK(idx->pq->k == 256, VG_ERR_UNSUPPORTED, "%s: LUT scan needs numCentroids == 256 (got %d)", fn, idx->pq->k);
    } else {
        VG_CHECK(idx->sq && (n == 0 || idx->d_sq_tiles), VG_ERR_NOT_READY, "%s: index has no SQ8 codes", fn);
    }
    VG_CHECK(!rerank || n == 0 || idx->d_vectors, VG_ERR_NOT_READY, "%s: rerank needs the fp32 vectors on the index", fn);
    if (nq == 0 || max_results == 0) return VG_OK;
    VG_CHECK(queries && thresholds && ids && scores && counts, VG_ERR_INVALID_ARG, "%s: NULL buffer", fn);
    VG_CHECK_MASK_STRIDE(fn, mask, mask_stride, n);
    vg::ThrIO io;
    VG_TRY(io.init(idx, stream, queries, nq, thresholds, max_results, mask, mask_stride, ids, scores, counts));
    hipStream_t st = io.st;
    const bool dot = idx->metric != VG_METRIC_L2;  // (the heap direction of EVERY scan follows the metric: flat/segment.go:449)
    const int dim = idx->dim;

    // bound form (b): the threshold says nothing about code scores (test hook: also without rerank, then the filter by scan score)
    const bool rerank_codes = rerank && scan != VG_SCAN_F32;
    const bool use_hist = rerank_codes || (!rerank && vg::hook(vg::kHookPthrForceHist));
    const int qb = whole && scan != VG_SCAN_PQ ? vg::kThrQB : 1;
    // the rows a query can see: the whole segment, or its np largest partitions at most
    int64_t list_cap = std::max<int64_t>(n, 1);
    if (!whole && static_cast<int>(idx->h_part_off.size()) == idx->num_partitions + 1) {
        std::vector<int64_t> sizes(static_cast<size_t>(idx->num_partitions));
        for (int p = 0; p < idx->num_partitions; p++) sizes[p] = static_cast<int64_t>(idx->h_part_off[p + 1]) - idx->h_part_off[p];
        std::partial_sort(sizes.begin(), sizes.begin() + np, sizes.end(), std::greater<int64_t>());
        int64_t sum = 0;
        for (int j = 0; j < np; j++) sum += sizes[j];
        list_cap = std::max<int64_t>(std::min(sum, n), 1);
    }
    // queries per launch: their lists stay below 2^25 keys (256 MiB), whole passes of kThrQB
    int64_t qc = std::min<int64_t>(64, std::max<int64_t>(1, (int64_t(1) << 25) / list_cap));
    if (qb > 1) qc = std::max<int64_t>(qb, qc / qb * qb);
    qc = std::min(qc, nq);
    const size_t uqc = static_cast<size_t>(qc);
    const int lut_words = scan == VG_SCAN_PQ ? vg::lut_image_words(idx->pq->m) : 0;
    int ranges, sub;
    vg::pthr_grid(idx, scan, whole ? 0 : np, qc, qb, ranges, sub);

    vg::ArenaCall ar(idx->ctx, st);
    const int i_lists = ar.add(sizeof(uint64_t) * uqc * list_cap);
    const int i_cnt = ar.add(sizeof(int) * uqc);
    const int i_hist = ar.add(use_hist ? sizeof(unsigned) * uqc * vg::kPthrBins : 0);
    const int i_cut = ar.add(sizeof(uint32_t) * uqc);
    const int i_probes = ar.add(whole ? 0 : sizeof(uint32_t) * static_cast<size_t>(nq) * np);
    const int i_tables = ar.add(sizeof(float) * uqc * lut_words);
    const int i_elist = ar.add(rerank_codes ? sizeof(uint64_t) * uqc * max_results : 0);
    const int i_ecount = ar.add(sizeof(int) * uqc);
    VG_TRY(ar.commit());
    uint64_t *lists = ar.get<uint64_t>(i_lists), *elist = ar.get<uint64_t>(i_elist);
    int *cnt = ar.get<int>(i_cnt), *ecount = ar.get<int>(i_ecount);
    unsigned *hist = ar.get<unsigned>(i_hist);
    uint32_t *cut = ar.get<uint32_t>(i_cut);
    uint32_t *probes = whole ? nullptr : ar.get<uint32_t>(i_probes);
    float *tables = ar.get<float>(i_tables);
    const uint32_t *part_off = whole ? nullptr : idx->d_part_off;

    if (!whole) VG_TRY(vg::launch_probe_select(idx, io.q.ptr, nq, np, dot, probes, st));
    // step 1, the candidate stage: per query the best max_results rows it can see (form a: of those within its threshold)
    for (int64_t q0 = 0; q0 < nq; q0 += qc) {
        const int64_t c = std::min(qc, nq - q0);
        VG_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * static_cast<size_t>(c), st));
        if (n > 0) {
            if (scan == VG_SCAN_PQ) VG_TRY(vg::launch_pq_build_table(idx->pq, io.q.ptr + q0 * dim, c, tables, true, st));
            const vg::PthrArgs a{io.q.ptr + q0 * dim, nullptr, dim, c, n, probes ? probes + q0 * np : nullptr, part_off, ranges, sub,
                                 io.t.ptr + q0, cut, io.mk.ptr ? io.mk.ptr + q0 * mask_stride : nullptr, mask_stride, list_cap, lists, cnt, hist};
            vg::ProfScope prof(idx->ctx, "probed_thr_scan", st);
            if (use_hist) {
                VG_HIP(hipMemsetAsync(hist, 0, sizeof(unsigned) * static_cast<size_t>(c) * vg::kPthrBins, st));
                VG_TRY(vg::pthr_pass(idx, scan, qb, tables, vg::kPthrHist, a, st));
                VG_LAUNCH(vg::pthr_cut_kernel, dim3(static_cast<unsigned>(c)), dim3(1024), 0, st, hist, max_results, cut);
                VG_TRY(vg::pthr_pass(idx, scan, qb, tables, vg::kPthrBin, a, st));
            } else {
                VG_TRY(vg::pthr_pass(idx, scan, qb, tables, vg::kPthrThr, a, st));
            }
        }
        vg::ProfScope prof(idx->ctx, "probed_thr_select", st);
        VG_TRY(vg::launch_thr_select_lists(dot, lists, list_cap, cnt, nullptr, c, list_cap, max_results, io.oid.ptr + q0 * max_results,
                                           io.osc.ptr + q0 * max_results, io.ocnt.ptr + q0, st));
    }
    if (n > 0) {
        // queries whose scan scores may hold a NaN: flat.Segment.Search(q, max_results) as its heap answers it, over the same ranges
        if (scan == VG_SCAN_SQ8)
            VG_TRY(vg::sq8_nan_replay(idx, io.q.ptr, nq, max_results, io.mk.ptr, mask_stride, probes, np, part_off, io.oid.ptr, io.osc.ptr, st));
        else if (scan == VG_SCAN_PQ)
            VG_TRY(vg::pq_nan_replay(idx, io.q.ptr, nq, max_results, dot, io.mk.ptr, mask_stride, probes, np, part_off, io.oid.ptr, io.osc.ptr, st));
        else
            VG_TRY(vg::launch_cand_replay(vg::FlatF32Scorer{idx->d_vectors, idx->d_norm_max + 1, dim, dot, 0}, io.q.ptr, dim, n, nq, max_results,
                                          dot, io.mk.ptr, mask_stride, io.oid.ptr, io.osc.ptr, st, nullptr, probes, np, part_off));
        if (rerank_codes) {
            // step 2, Segment.Rerank: every candidate's exact score; step 3 fused: those within the threshold, best first
            for (int64_t q0 = 0; q0 < nq; q0 += qc) {
                const int64_t c = std::min(qc, nq - q0);
                vg::ProfScope prof(idx->ctx, "probed_thr_rerank", st);
                VG_TRY(vg::launch_thr_rescore(dot, idx->d_vectors, dim, io.q.ptr + q0 * dim, io.t.ptr + q0, nullptr, nullptr,
                                              io.oid.ptr + q0 * max_results, c, max_results, elist, ecount, st));
                VG_TRY(vg::launch_thr_select_lists(dot, elist, max_results, ecount, nullptr, c, max_results, max_results,
                                                   io.oid.ptr + q0 * max_results, io.osc.ptr + q0 * max_results, io.ocnt.ptr + q0, st));
            }
        } else {
            // step 3 over what the replay or form (b) left (idempotent on form (a)'s lists)
            VG_TRY(vg::launch_thr_filter(dot, io.t.ptr, nq, max_results, io.oid.ptr, io.osc.ptr, io.ocnt.ptr, st));
        }
    }
    return io.finish();
}
