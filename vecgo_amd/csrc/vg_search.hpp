// vg_search.hpp — what the search translation units share on the host: every function one .hip defines and another calls,
// declared once (the defining file includes this header too, so a definition that disagrees does not compile), and the
// scaffolding every search entry point stands on: SearchIO (staged operands), empty_results, PagedTopK (k > 64 in pages),
// for the flat threshold searches ThrIO (SearchIO + thresholds and counts), their constants and metric dispatch,
// and for the graph walks WalkIO (SearchIO + per-query counters) and WalkChunks (per-query scratch, a batch in launches).
// (The bf16 nomination's functions are declared in vg_nominate.hpp.)
#pragma once

#include <algorithm>
#include <type_traits>

#include "vg_internal.hpp"
#include "vg_walk_chunk.hpp"

namespace vg {

// ---- k_topk_merge.hip -----------------------------------------------------------------------------
// the merge kernels' workgroup and LDS key buffer (topk_merge_kernel; topk_select_verify_kernel, k_adc.hip), and the largest k they
// take: vg_search_pq_adc's and vg_merge_topk's limit
constexpr int kMergeThreads = 256;
constexpr int kMergeBuf = 4096;
constexpr int kAdcMaxK = 1024;
// per query the k best of `lists` k-lists of keys -> ids / scores; only_if[q] == 0 leaves query q alone unless always[0] != 0
int32_t launch_topk_merge(const uint64_t *partial, int64_t nq, int lists, int k, bool descending,
                          uint32_t *ids, float *scores, hipStream_t st, const int *only_if = nullptr,
                          const int *always = nullptr);

// ---- k_adc.hip ------------------------------------------------------------------------------------
// row-major PQ codes -> the scan's tiles (vg_vamana_reorder_bfs rebuilds them from its permuted codes)
int32_t launch_pq_retile(const uint8_t *codes, int64_t n, int m, int groups, int64_t n_tiles, uint8_t *tiles, hipStream_t st);
// the probed partitions' rows by table lookups, `split` k-lists per query
int32_t launch_probe_scan_adc(const vg_index *idx, const float *tables, const uint32_t *probes, const uint32_t *part_off,
                              int64_t nq, int np, int split, int k, uint64_t *partial, const uint64_t *min_keys, bool desc,
                              const uint8_t *mask, int64_t mask_stride, hipStream_t st);
// the replay for device buffers: the whole segment, or (probes: nq * np partition ids, part_off) the probed partitions; mask: a
// device row filter per query / for the batch, or null; desc: a Dot / Cosine segment keeps the LARGEST sums (flat/segment.go:449)
int32_t pq_nan_replay(vg_index *idx, const float *d_queries, int64_t nq, int k, bool desc, const uint8_t *d_mask, int64_t mask_stride,
                      const uint32_t *d_probes, int np, const uint32_t *d_part_off, uint32_t *d_ids, float *d_scores, hipStream_t st);
// vg_search_pq_adc with a DEVICE row filter (null: none) and the heap direction given
int32_t pq_adc_search_masked(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask, int64_t mask_stride,
                             bool desc, uint32_t *ids, float *scores, void *stream);

// ---- k_hnsw_predicate.hip -------------------------------------------------------------------------
// the index's layer-0 edge distances (Neighbor.Dist): uploaded from l0_dist, or (null) recomputed from the rows by the pair kernel
int32_t hnsw_edge_distances(vg_index *idx, const float *l0_dist, hipStream_t st);

// ---- k_pq.hip -------------------------------------------------------------------------------------
// the queries' distance tables, in the ADC scan's LDS layout (scan_layout) or [m][k]
int32_t launch_pq_build_table(const vg_pq *pq, const float *d_queries, int64_t nq, float *d_tables,
                              bool scan_layout, hipStream_t st);

// ---- k_flat.hip -----------------------------------------------------------------------------------
// all queries of a paged scan (k > 64 through a kernel that keeps 64 keys per wave): copy page `off / 64` and
// make its last key the floor of the next page
int32_t launch_page_patch(int64_t nq, int k, int off, int kk, bool descending, const int *always_one,
                          const uint32_t *fids, const float *fscores, uint32_t *ids, float *scores, uint64_t *min_keys,
                          hipStream_t st);
// vg_search_flat with a DEVICE row filter (null: none); l2_scores: squared-L2 scores whatever the index's metric;
// cand_replay: the NaN replay of vg_cand_replay.hpp at the end (a caller that replays for itself passes false)
int32_t flat_search_masked(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask, int64_t mask_stride,
                           uint32_t *ids, float *scores, void *stream, bool l2_scores = false, bool cand_replay = true);
// the bfloat16 filter's share of a proof's margin (a multiple of |q|^2 + max |x|^2)
float bf16_filter_eps(bool dot);
// The threshold search's nomination (k_flat_threshold.hip).  The plan: appended keys kept per query, thresholds kept per query,
// every sample_stride-th row tile sampled, nomination on the bf16 filter's rows, the proof's extra margin.
struct ThrNomPlan {
    int cap, sel_k, sample_stride;
    bool bf16;
    float eps_extra;
};
// its outputs, in the scratch: [cnt] each, cand [cnt * cap] GEMM keys
struct ThrNominated {
    float *gthr, *qnorm;
    int *untight, *counts;
    uint64_t *cand;
};
// scratch: flat_thr_nominate_scratch bytes of the caller's arena, for chunks of up to qc queries
size_t flat_thr_nominate_scratch(const vg_index *idx, const ThrNomPlan &plan, int64_t qc);
int32_t flat_thr_nominate(vg_index *idx, const ThrNomPlan &plan, const float *qp, const float *uthr, int64_t cnt, const uint8_t *m0,
                          int64_t mask_stride, char *scratch, ThrNominated *out, hipStream_t st);
int32_t launch_flat_todo(const int *flags, const int *always, int cnt, int *todo, unsigned long long *stats, hipStream_t st,
                         const int *counts = nullptr);

// ---- the threshold searches: k_flat_threshold.hip, k_probed_threshold.hip (and the large-k Vamana walk, k_graph.hip) ----
constexpr int kThrMaxResults = 16384;  // the selection's LDS buffer (128 KiB of keys) and the replay's heap
constexpr int kThrQB = 8;              // queries one pass over the whole segment carries (fp32, SQ8)
// the register form of the exact scan: rows of whole float4 (dim % 4 == 0, 16-byte aligned), up to 16 float4 per lane
inline bool thr_scan_regs(const vg_index *idx)
{
    return idx->dim % 4 == 0 && idx->dim >= 64 && idx->dim <= 1024 && aligned16(idx->d_vectors);
}
// the metric of a launch as a compile-time constant: f(std::true_type) for Dot / Cosine, f(std::false_type) for L2
template <class F>
inline int32_t with_metric(bool dot, F f)
{
    return dot ? f(std::true_type{}) : f(std::false_type{});
}
// k_flat_threshold.hip.  The best max_results keys of `nq` lists (list s: counts[s] keys at lists + s * list_cap), written best
// first to query qmap[s] (null: s) of ids / scores / out_counts; `longest`: no list holds more keys.  A list of up to 16384
// keys is sorted whole in LDS, a longer one radix-selects its max_results-th key first.
int32_t launch_thr_select_lists(bool desc, const uint64_t *lists, int64_t list_cap, const int *counts, const int *qmap, int64_t nq,
                                int64_t longest, int max_results, uint32_t *ids, float *scores, int32_t *out_counts, hipStream_t st);
// the engine's filter over each query's results, in order
int32_t launch_thr_filter(bool desc, const float *thr, int64_t nq, int max_results, uint32_t *ids, float *scores, int32_t *counts,
                          hipStream_t st);
// Exact scores of candidate rows, those within each query's threshold as keys in lists[nq * cap] / list_counts[nq] (zeroed
// here).  cand_ids null: the rows of the nomination's keys, cand_counts[q] (at most cap) of cand[q * cap ..]; else a search's
// result rows cand_ids[nq * cap], VG_INVALID_ID where unused (Segment.Rerank's input)
int32_t launch_thr_rescore(bool desc, const float *base, int dim, const float *queries, const float *thr, const uint64_t *cand,
                           const int *cand_counts, const uint32_t *cand_ids, int64_t nq, int cap, uint64_t *lists, int *list_counts,
                           hipStream_t st);
// k_probed_threshold.hip.  One exact fp32 pass over the whole segment for `cnt` slots, kThrQB per workgroup: slot s scores
// every row against query qmap[s] (null: s) of queries / thr / mask and appends the keys within its threshold and filter to
// list s (lists + s * list_cap, counts[s]; the caller zeroes the counts)
int32_t launch_thr_scan_f32(const vg_index *idx, const float *queries, const float *thr, const int *qmap, int64_t cnt,
                            const uint8_t *mask, int64_t mask_stride, int64_t list_cap, uint64_t *lists, int *counts, hipStream_t st);

// ---- k_probe.hip ----------------------------------------------------------------------------------
// kmeans.FindClosestCentroids for every query (device buffers): probes[q * np + j]
int32_t launch_probe_select(const vg_index *idx, const float *d_queries, int64_t nq, int np, bool dot, uint32_t *d_probes, hipStream_t st);

// ---- k_sq8.hip ------------------------------------------------------------------------------------
// stage 1 of a quantizer's Train (SQ8, INT4) over device rows: per-dimension min / max of min(n, 1024) row chunks,
// pmin / pmax [chunks][dim] allocated here for the caller's finish kernel
int32_t launch_dim_minmax(const float *d_rows, int64_t n, int dim, DevTmp<float> &pmin, DevTmp<float> &pmax, int &chunks,
                          hipStream_t st);

// ---- k_sq8_scan.hip -------------------------------------------------------------------------------
// the probed partitions' rows from the SQ8 codes: one pass per (query, probe), or per group of pairs of one partition
int32_t launch_probe_scan_sq8(const vg_index *idx, const float *queries, const uint32_t *probes, const uint32_t *part_off,
                              int64_t nq, int np, int sub, int k, uint64_t *partial, const uint64_t *min_keys,
                              const uint8_t *mask, int64_t mask_stride, hipStream_t st);
int32_t launch_probe_scan_sq8_grouped(const vg_index *idx, const float *queries, const uint32_t *part_off,
                                      const uint32_t *pair_of, const ProbeGroup *groups, const uint32_t *ngroups, unsigned gmax,
                                      int np, int sub, int k, uint64_t *partial, const uint64_t *min_keys, const uint8_t *mask,
                                      int64_t mask_stride, hipStream_t st);
// pq_nan_replay's twin (the heap direction follows the index's metric)
int32_t sq8_nan_replay(vg_index *idx, const float *d_queries, int64_t nq, int k, const uint8_t *d_mask, int64_t mask_stride,
                       const uint32_t *d_probes, int np, const uint32_t *d_part_off, uint32_t *d_ids, float *d_scores, hipStream_t st);

// ---- k_vamana_build.hip ---------------------------------------------------------------------------
// vg_vamana_build's defaults (r, l, alpha of 0) and every refusal it makes before it allocates, with its status and message
int32_t vamana_build_check(const vg_index *idx, int32_t &r, int32_t &l, float &alpha, int32_t max_batch, int32_t growth_div);

// ---- k_rabitq.hip ---------------------------------------------------------------------------------
// sign bits + norm of each vector (RaBitQ Encode)
int32_t launch_rabitq_encode(const float *d_vectors, int64_t n, int dim, uint8_t *d_codes, hipStream_t st);
// row-major codes -> the scan's tiles and norms[0, n) (vg_vamana_reorder_bfs rebuilds them from its permuted codes)
int32_t launch_rabitq_retile(const uint8_t *codes, int64_t n, int nb, int groups, int64_t n_tiles, uint8_t *tiles, float *norms,
                             hipStream_t st);

// ---- the scaffolding of a search entry point ------------------------------------------------------
// The operands of one search call: the device, the stream, the queries (and a row filter) staged into HBM when they live on the
// host, ids / scores produced in HBM.  finish() copies the results back and waits for them where they went to the host.
struct SearchIO {
    hipStream_t st = nullptr;
    DevIn<float> q;
    DevIn<uint8_t> mk;
    DevOut<uint32_t> oid;
    DevOut<float> osc;
    int32_t init(vg_ctx *ctx, void *stream, const float *queries, size_t query_floats, uint32_t *ids, float *scores, size_t results,
                 const uint8_t *mask = nullptr, size_t mask_bytes = 0, Align align = kStage16)
    {
        // align: kAnyAlign only for the library's own sub-ranges of operands an outer SearchIO has already taken
        VG_HIP(hipSetDevice(ctx->device));
        st = pick_stream(ctx, stream);
        VG_TRY(q.init(queries, query_floats, st, align));
        VG_TRY(oid.init(ids, results, st, align));
        VG_TRY(osc.init(scores, results, st, align));
        return mk.init(mask, mask_bytes, st, align);
    }
    int32_t finish()
    {
        VG_TRY(oid.finish());
        return osc.finish();
    }
};

// The walks' operands: SearchIO and the per-query counters (null: not asked for).
struct WalkIO : SearchIO {
    DevOut<vg_search_stats> ost;
    int32_t init(vg_ctx *ctx, void *stream, const float *queries, size_t query_floats, uint32_t *ids, float *scores, size_t results,
                 vg_search_stats *stats, int64_t nq, const uint8_t *mask = nullptr, size_t mask_bytes = 0)
    {
        VG_TRY(SearchIO::init(ctx, stream, queries, query_floats, ids, scores, results, mask, mask_bytes));
        return ost.init(stats, stats ? static_cast<size_t>(nq) : 0, st);
    }
    vg_search_stats *stats_at(int64_t q0) const { return ost.ptr ? ost.ptr + q0 : nullptr; }
    int32_t finish()
    {
        VG_TRY(SearchIO::finish());
        return ost.finish();
    }
};

// the bytes of nq row filters of an n-row index, mask_stride apart (0: one filter for the batch); no filter: 0
inline size_t mask_span(const uint8_t *mask, int64_t mask_stride, int64_t nq, int64_t n)
{
    const int64_t mask_bytes = (n + 7) / 8;
    return mask ? static_cast<size_t>(mask_stride ? (nq - 1) * mask_stride + mask_bytes : mask_bytes) : 0;
}

// The flat threshold searches' operands: SearchIO (max_results ids / scores per query), a threshold per query and the counts.
struct ThrIO : SearchIO {
    DevIn<float> t;
    DevOut<int32_t> ocnt;
    int32_t init(const vg_index *idx, void *stream, const float *queries, int64_t nq, const float *thresholds, int max_results,
                 const uint8_t *mask, int64_t mask_stride, uint32_t *ids, float *scores, int32_t *counts)
    {
        VG_TRY(SearchIO::init(idx->ctx, stream, queries, static_cast<size_t>(nq) * idx->dim, ids, scores,
                              static_cast<size_t>(nq) * max_results, mask, mask_span(mask, mask_stride, nq, idx->n)));
        VG_TRY(t.init(thresholds, static_cast<size_t>(nq), st));
        return ocnt.init(counts, static_cast<size_t>(nq), st);
    }
    int32_t finish()
    {
        VG_TRY(SearchIO::finish());
        return ocnt.finish();
    }
};

// a filter per query (mask_stride != 0) has to be at least a filter long; `fn`: the entry point the message names
#define VG_CHECK_MASK_STRIDE(fn, mask, mask_stride, n)                                                                              \
    VG_CHECK((mask) == nullptr || (mask_stride) == 0 || (mask_stride) >= ((n) + 7) / 8, VG_ERR_INVALID_ARG,                         \
             "%s: mask_stride %lld is shorter than a mask (%lld bytes)", fn, static_cast<long long>(mask_stride),                   \
             static_cast<long long>(((n) + 7) / 8))

// Per-query scratch of the graph searches (visited bitmap, HBM part of the heaps, exploration heap) is carved from
// the arena for as many queries as fit under this cap; the rest of the batch goes into further launches.  1 GiB (r02)
// cut 8192 Vamana queries over 1M nodes (650 KB each) into 5 launches of 1650 wavefronts — fewer than the 3072 the
// chip holds.  1/16 of the device's memory, at most 16 GiB.
inline int64_t scratch_cap(const vg_ctx *ctx)
{
    const int64_t gib = int64_t(1) << 30;
    return std::min<int64_t>(16 * gib, std::max<int64_t>(gib, ctx->hbm_bytes / 16));
}

// `count` graph walks in launches of at most `chunk` (walk_chunk, vg_walk_chunk.hpp), vis holding `chunk` visited bitmaps of
// vis_words words: body(q0, cnt) walks q0 .. q0 + cnt - 1 over cleared bitmaps; the first status that is not VG_OK ends the batch
template <class Body>
inline int32_t for_each_walk_chunk(uint32_t *vis, int64_t vis_words, int64_t chunk, int64_t count, hipStream_t st, Body body)
{
    for (int64_t q0 = 0; q0 < count; q0 += chunk) {
        const int64_t cnt = std::min(chunk, count - q0);
        VG_HIP(hipMemsetAsync(vis, 0, static_cast<size_t>(cnt) * vis_words * 4, st));
        VG_TRY(body(q0, cnt));
    }
    return VG_OK;
}

// A batch of graph walks in launches of `chunk` queries (for_each_walk_chunk), each query with a visited bitmap of
// vis_words words of its own.  other_bytes: a query's scratch besides the bitmap.  add() before the arena's commit() — the
// caller's pieces are chunk times a query's —, for_each() after it.  The test hook VG_WALK_SMALL_SCRATCH caps a launch at
// kWalkHookChunk queries, so that a test batch takes the several launches a batch over a large graph takes.
constexpr int64_t kWalkHookChunk = 5;
struct WalkChunks {
    int64_t nq, vis_words, chunk;
    const ArenaCall *ar = nullptr;
    int i_vis = 0;
    WalkChunks(int64_t cap, int64_t other_bytes, int64_t n, int64_t nq_)
        : nq(nq_), vis_words((n + 31) / 32), chunk(walk_chunk(cap, vis_words * 4 + other_bytes, nq_))
    {
        if (hook(kHookWalkSmallScratch)) chunk = std::min(chunk, kWalkHookChunk);
    }
    void add(ArenaCall &a)
    {
        ar = &a;
        i_vis = a.add(sizeof(uint32_t) * static_cast<size_t>(chunk) * vis_words);
    }
    uint32_t *vis() const { return ar->get<uint32_t>(i_vis); }
    template <class Body>
    int32_t for_each(hipStream_t st, Body body) const
    {
        return for_each_walk_chunk(vis(), vis_words, chunk, nq, st, body);
    }
};

// The answer of an index without rows: k invalid ids per query, through the merge every scan ends in.
inline int32_t empty_results(int64_t nq, int k, bool descending, uint32_t *ids, float *scores, hipStream_t st)
{
    DevTmp<uint64_t> none;
    VG_TRY(none.init(static_cast<size_t>(nq) * k, st));
    VG_HIP(hipMemsetAsync(none.ptr, 0xFF, static_cast<size_t>(nq) * k * 8, st));
    return launch_topk_merge(none.ptr, nq, 1, k, descending, ids, scores, st);
}

// A scan whose waves keep 64 keys answers k > 64 in pages of 64 results, each page a scan for the keys after the previous
// page's last one (ceil(k / 64) scans); k <= 64 is the one scan, merged straight into the results.  add() before the arena's
// commit(), run() after it.  scan(kk, partial, floor): fills `lists` kk-lists per query in `partial`; floor[q] (null on the
// first page) is the key the page's keys have to follow.
struct PagedTopK {
    int64_t nq = 0;
    int k = 0;
    int i_partial = 0, i_pid = 0, i_psc = 0, i_floor = 0, i_one = 0;
    bool paged() const { return k > 64; }
    // min_partial_keys: what else the caller keeps in `partial`
    void add(ArenaCall &ar, int64_t nq_, int k_, int lists, size_t min_partial_keys = 0)
    {
        nq = nq_;
        k = k_;
        const int pk = paged() ? 64 : k;
        i_partial = ar.add(sizeof(uint64_t) * std::max(static_cast<size_t>(nq) * lists * pk, min_partial_keys));
        i_pid = ar.add(paged() ? sizeof(uint32_t) * static_cast<size_t>(nq) * pk : 0);
        i_psc = ar.add(paged() ? sizeof(float) * static_cast<size_t>(nq) * pk : 0);
        i_floor = ar.add(paged() ? sizeof(uint64_t) * static_cast<size_t>(nq) : 0);
        i_one = ar.add(paged() ? 256 : 0);
    }
    template <class Scan>
    int32_t run(const ArenaCall &ar, int lists, bool descending, uint32_t *ids, float *scores, hipStream_t st, Scan scan) const
    {
        uint64_t *partial = ar.get<uint64_t>(i_partial), *floor_keys = ar.get<uint64_t>(i_floor);
        uint32_t *pid = ar.get<uint32_t>(i_pid);
        float *psc = ar.get<float>(i_psc);
        int *one = ar.get<int>(i_one);
        if (paged()) VG_HIP(hipMemsetAsync(one, 1, sizeof(int), st));
        for (int off = 0; off < k; off += 64) {
            const int kk = paged() ? std::min(64, k - off) : k;
            VG_TRY(scan(kk, partial, off ? floor_keys : nullptr));
            if (!paged()) {
                VG_TRY(launch_topk_merge(partial, nq, lists, k, descending, ids, scores, st));
            } else {
                VG_TRY(launch_topk_merge(partial, nq, lists, kk, descending, pid, psc, st));
                VG_TRY(launch_page_patch(nq, k, off, kk, descending, one, pid, psc, ids, scores, floor_keys, st));
            }
        }
        return VG_OK;
    }
};

}  // namespace vg
