// k_flat_threshold.hip — Engine.SearchThreshold over one flat segment (engine/engine.go:1485-1531):
//   flat.Segment.Search(q, k = max_results) (flat/segment.go:447-721, fp32 branch), then the rows with
//   Score <= threshold (L2) / Score >= threshold (Dot, Cosine), best first.
//   1. one pass over the rows scores every row against up to 8 queries in the reference's summation order and
//      appends the key (score bits, row id) of every row whose EXACT score passes its query's threshold to that
//      query's list in HBM (n keys per query: it cannot overflow, nothing is left to prove): launch_thr_scan_f32, the
//      probed threshold search's exact scan (k_probed_threshold.hip)
//   2. per query the best min(count, max_results) keys of its list: a bitonic sort in LDS, or — a list longer
//      than the LDS buffer — a radix select of the max_results-th key over the list first
//   3. queries whose scores may hold a NaN: the reference's heap replayed with k = max_results (vg_cand_replay.hpp),
//      then the engine's filter over what it pops
#include <algorithm>

#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_cand_replay.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"

namespace vg {

constexpr int kThrSelThreads = 1024;
constexpr int kThrSelWaves = kThrSelThreads / 64;

// the engine's filter (engine.go:1518-1529): both comparisons keep the boundary; NaN on either side keeps nothing
template <bool DOT>
__device__ __forceinline__ bool thr_keep(float score, float t)
{
    return DOT ? score >= t : score <= t;
}

// ---- 2. selection: the best min(count, max_results) keys of a list, in order ----------------------------------------
// One workgroup per list (query qmap[blockIdx.x], null: blockIdx.x); `sbuf` keys of LDS (a power of two, >= max_results).  A list that
// fits is sorted whole; a longer one first finds its max_results-th key by eight 8-bit digit passes over HBM (keys are
// unique: a row appears once per list), then sorts the max_results keys at or below it.
template <bool DOT>
__global__ __launch_bounds__(kThrSelThreads) void flat_thr_select_kernel(const uint64_t *__restrict__ lists, int64_t list_cap,
                                                                         const int *__restrict__ counts, int max_results, int sbuf,
                                                                         const int *__restrict__ qmap, uint32_t *__restrict__ ids,
                                                                         float *__restrict__ scores, int32_t *__restrict__ out_counts)
{
    extern __shared__ uint64_t sel_lds[];  // sbuf keys, then a digit histogram per wave (the column sums land in wave 0's)
    unsigned *hist = reinterpret_cast<unsigned *>(sel_lds + sbuf);
    __shared__ uint64_t prefix_s;
    __shared__ int rank_s, fill_s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int64_t slot = blockIdx.x, q = qmap ? qmap[slot] : slot;
    const uint64_t *src = lists + slot * list_cap;
    const int64_t c = counts[slot] < list_cap ? counts[slot] : list_cap;
    int m;  // keys in LDS after this step, all of them wanted
    if (c <= sbuf) {
        m = static_cast<int>(c);
        for (int i = tid; i < m; i += kThrSelThreads) sel_lds[i] = src[i];
    } else {
        uint64_t prefix = 0, pmask = 0;
        int rank = max_results - 1;  // rank of the wanted key among those matching the prefix
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int b = tid; b < kThrSelWaves * 256; b += kThrSelThreads) hist[b] = 0;
            __syncthreads();
            for (int64_t i = tid; i < c; i += kThrSelThreads) {
                const uint64_t key = src[i];
                if ((key & pmask) == prefix) atomicAdd(&hist[wave * 256 + ((key >> shift) & 255)], 1u);
            }
            __syncthreads();
            if (tid < 256) {
                unsigned sum = 0;
                for (int w = 0; w < kThrSelWaves; w++) sum += hist[w * 256 + tid];
                hist[tid] = sum;
            }
            __syncthreads();
            if (tid == 0) {
                int b = 0;
                for (; b < 255; b++) {
                    if (rank < static_cast<int>(hist[b])) break;
                    rank -= static_cast<int>(hist[b]);
                }
                prefix_s = prefix | (static_cast<uint64_t>(b) << shift);
                rank_s = rank;
            }
            __syncthreads();
            prefix = prefix_s;
            rank = rank_s;
            pmask |= uint64_t(255) << shift;
        }
        // prefix is now the max_results-th key: exactly max_results keys are <= it
        if (tid == 0) fill_s = 0;
        __syncthreads();
        for (int64_t i = tid; i < c; i += kThrSelThreads) {
            const uint64_t key = src[i];
            if (key <= prefix) sel_lds[atomicAdd(&fill_s, 1)] = key;
        }
        m = max_results;
    }
    int n2 = 2;
    while (n2 < m) n2 <<= 1;
    for (int i = m + tid; i < n2; i += kThrSelThreads) sel_lds[i] = kKeyMax;
    __syncthreads();
    bitonic_sort_lds(sel_lds, n2, tid, kThrSelThreads);
    const int kept = m < max_results ? m : max_results;
    for (int i = tid; i < max_results; i += kThrSelThreads) {
        const uint64_t e = i < kept ? sel_lds[i] : kKeyMax;
        ids[q * max_results + i] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        scores[q * max_results + i] = e == kKeyMax ? (DOT ? -INFINITY : INFINITY) : key_score(e, DOT);
    }
    if (tid == 0) out_counts[q] = kept;
}

// ---- 3. the engine's filter over a query's results, in order (after the heap replay; idempotent on the lists' answer) --
template <bool DOT>
__global__ __launch_bounds__(64) void flat_thr_filter_kernel(const float *__restrict__ thr, int max_results, uint32_t *__restrict__ ids,
                                                             float *__restrict__ scores, int32_t *__restrict__ out_counts)
{
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const float t = thr[q];
    uint32_t *qi = ids + q * max_results;
    float *qs = scores + q * max_results;
    int kept = 0;
    for (int i0 = 0; i0 < max_results; i0 += 64) {
        const int i = i0 + lane;
        const uint32_t id = i < max_results ? qi[i] : VG_INVALID_ID;
        const float sc = i < max_results ? qs[i] : 0.0f;
        const bool keep = id != VG_INVALID_ID && thr_keep<DOT>(sc, t);
        const uint64_t m = __ballot(keep);
        if (keep) {  // (kept + rank <= i: every lane has read its slot before any lane writes)
            const int at = kept + __popcll(m & ((uint64_t(1) << lane) - 1));
            qi[at] = id;
            qs[at] = sc;
        }
        kept += __popcll(m);
    }
    for (int i = kept + lane; i < max_results; i += 64) {
        qi[i] = VG_INVALID_ID;
        qs[i] = DOT ? -INFINITY : INFINITY;
    }
    if (lane == 0) out_counts[q] = kept;
}

// the two steps above, for this file's lists and for those another search fills: the probed scans' (k_probed_threshold.hip) and
// the result heap vg_search_vamana's large-k walk leaves as a list of k keys (kKeyMax after the last)
int32_t launch_thr_select_lists(bool desc, const uint64_t *lists, int64_t list_cap, const int *counts, const int *qmap, int64_t nq,
                                int64_t longest, int max_results, uint32_t *ids, float *scores, int32_t *out_counts, hipStream_t st)
{
    if (nq == 0) return VG_OK;
    int sbuf = 64;  // the LDS keys: the longest list that can occur, at least max_results, at most kThrMaxResults
    while (sbuf < std::max<int64_t>(max_results, std::min<int64_t>(longest, kThrMaxResults))) sbuf <<= 1;
    const size_t hist = kThrSelWaves * 256 * sizeof(unsigned);
    return with_metric(desc, [&](auto dot) -> int32_t {
        auto sel = flat_thr_select_kernel<decltype(dot)::value>;
        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(sizeof(uint64_t) * kThrMaxResults + hist)));
        VG_LAUNCH(sel, dim3(static_cast<unsigned>(nq)), dim3(kThrSelThreads), sizeof(uint64_t) * static_cast<size_t>(sbuf) + hist, st, lists,
                  list_cap, counts, max_results, sbuf, qmap, ids, scores, out_counts);
        return VG_OK;
    });
}

int32_t launch_thr_filter(bool desc, const float *thr, int64_t nq, int max_results, uint32_t *ids, float *scores, int32_t *counts,
                          hipStream_t st)
{
    if (nq == 0) return VG_OK;
    return with_metric(desc, [&](auto dot) -> int32_t {
        VG_LAUNCH(flat_thr_filter_kernel<decltype(dot)::value>, dim3(static_cast<unsigned>(nq)), dim3(64), 0, st, thr, max_results, ids,
                  scores, counts);
        return VG_OK;
    });
}

// ---- batches: the rows the nomination appended (GEMM keys), re-scored exactly; those within the threshold go to the list ---------
// grid (workgroups per query, queries); 4 candidates per wave step, one per 16-lane group
// cand_ids (null: the keys of `cand`, counts[q] each): a search's result rows instead, cap per query, VG_INVALID_ID where a
// slot is unused — Segment.Rerank's input after a scan over codes (k_probed_threshold.hip)
template <bool DOT>
__global__ __launch_bounds__(256) void flat_thr_rescore_kernel(const float *__restrict__ base, int dim, const float *__restrict__ queries,
                                                               const float *__restrict__ thr, const uint64_t *__restrict__ cand,
                                                               const uint32_t *__restrict__ cand_ids, const int *__restrict__ counts,
                                                               int cap, uint64_t *__restrict__ lists, int *__restrict__ list_counts)
{
    const int64_t q = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Sub16 sub = Sub16::make(tid);
    const int c = cand_ids ? cap : (counts[q] < cap ? counts[q] : cap);
    if (c == 0) return;
    const float *qv = queries + q * dim;
    const float t = thr[q];
    for (int c0 = blockIdx.x * 16 + wave * 4; c0 < c; c0 += gridDim.x * 16) {
        const int ci = c0 + (lane >> 4);
        bool live = ci < c;
        uint32_t id = cand_ids ? cand_ids[q * cap + (live ? ci : c - 1)] : key_row(cand[q * cap + (live ? ci : c - 1)]);
        if (cand_ids && id == VG_INVALID_ID) {
            live = false;
            id = 0;
        }
        const float v = exact_pair16<DOT, kPair>(base + static_cast<int64_t>(id) * dim, qv, dim, sub);
        const bool pass = live && (lane & 15) == 0 && thr_keep<DOT>(v, t);
        wave_append(pass, make_key(v, id, DOT), list_counts + q, lists + q * cap, lane);
    }
}

int32_t launch_thr_rescore(bool desc, const float *base, int dim, const float *queries, const float *thr, const uint64_t *cand,
                           const int *cand_counts, const uint32_t *cand_ids, int64_t nq, int cap, uint64_t *lists, int *list_counts,
                           hipStream_t st)
{
    if (nq == 0 || cap == 0) return VG_OK;
    VG_HIP(hipMemsetAsync(list_counts, 0, sizeof(int) * static_cast<size_t>(nq), st));
    const dim3 grid(static_cast<unsigned>(std::min(32, std::max(1, cap / 2048))), static_cast<unsigned>(nq));
    return with_metric(desc, [&](auto dot) -> int32_t {
        VG_LAUNCH(flat_thr_rescore_kernel<decltype(dot)::value>, grid, dim3(256), 0, st, base, dim, queries, thr, cand, cand_ids,
                  cand_counts, cap, lists, list_counts);
        return VG_OK;
    });
}

// The proof of a nominated query (one thread per query).  The user's threshold stood (untight = 1) and the list did not
// overflow: every row within it was appended — the result is exact.  The sample tightened it (untight = 0): every row not
// appended has GEMM score >= gthr, i.e. an exact score at or beyond gthr (+ |q|^2 for L2) less the error bound; the result is
// exact if it holds max_results rows and the last of them is strictly better than that.  fail[q] = 1: the scan answers it.
template <bool DOT>
__global__ void flat_thr_proof_kernel(int64_t cnt, const int *__restrict__ untight, const int *__restrict__ counts, int cap,
                                      const float *__restrict__ gthr, const float *__restrict__ qnorm, const float *__restrict__ norm_max,
                                      int dim, float eps_extra, int max_results, const int32_t *__restrict__ out_counts,
                                      const float *__restrict__ scores, int *__restrict__ fail)
{
    const int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= cnt) return;
    bool ok = untight[q] >= 0 && counts[q] <= cap;
    if (ok && untight[q] == 0) {
        const float qn = qnorm[q], tau = gthr[q];
        const float eps = (4.0f * (static_cast<float>(dim) * 5.9604645e-8f) + eps_extra) * (qn + norm_max[0]) + 1e-30f;
        const float kth = scores[q * max_results + max_results - 1];
        ok = out_counts[q] == max_results && (DOT ? kth > (-tau) + eps : kth < (tau + qn) - eps);
    }
    fail[q] = ok ? 0 : 1;
}

__global__ void flat_thr_stats_kernel(unsigned long long *__restrict__ stats, long long searched, long long exact)
{
    if (threadIdx.x == 0) {
        atomicAdd(&stats[0], static_cast<unsigned long long>(searched));
        atomicAdd(&stats[1], static_cast<unsigned long long>(exact));
    }
}

}  // namespace vg

VG_API int32_t vg_search_flat_threshold(vg_index *idx, const float *queries, int64_t nq, const float *thresholds,
                                        int32_t max_results, const uint8_t *mask, int64_t mask_stride, uint32_t *ids,
                                        float *scores, int32_t *counts, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_search_flat_threshold: NULL index");
    VG_CHECK(nq >= 0 && max_results >= 0, VG_ERR_INVALID_ARG, "vg_search_flat_threshold: negative nq or max_results");
    VG_CHECK(max_results <= vg::kThrMaxResults, VG_ERR_UNSUPPORTED, "vg_search_flat_threshold: max_results=%d exceeds %d",
             max_results, vg::kThrMaxResults);
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    // a partitioned segment is searched over the nprobes closest partitions only (flat/segment.go:727-744)
    VG_CHECK(idx->num_partitions <= 1, VG_ERR_UNSUPPORTED,
             "vg_search_flat_threshold: the segment has %d IVF partitions (the reference probes only some of them)",
             idx->num_partitions);
    if (nq == 0 || max_results == 0) return VG_OK;
    VG_CHECK(queries && thresholds && ids && scores && counts, VG_ERR_INVALID_ARG, "vg_search_flat_threshold: NULL buffer");
    VG_CHECK(idx->n == 0 || idx->d_vectors, VG_ERR_NOT_READY, "vg_search_flat_threshold: index has no fp32 vectors");
    VG_CHECK_MASK_STRIDE("vg_search_flat_threshold", mask, mask_stride, idx->n);
    vg::ThrIO io;
    VG_TRY(io.init(idx, stream, queries, nq, thresholds, max_results, mask, mask_stride, ids, scores, counts));
    hipStream_t st = io.st;
    const bool dot = idx->metric != VG_METRIC_L2;
    const int64_t n = idx->n;
    const int dim = idx->dim;
    const int64_t list_cap = std::max<int64_t>(n, 1);
    // batches of more than kThrQB queries are nominated on the matrix cores (test hooks: VG_FLAT_NO_SCAN nominates every batch,
    // VG_FLAT_FORCE_EXACT scans every query); the rest, and the queries whose proof fails, take the scan
    const bool force_exact = vg::hook(vg::kHookFlatForceExact);
    const bool nominate = n > 0 && !force_exact && (nq > vg::kThrQB || vg::hook(vg::kHookFlatNoScan));
    const bool bf16 = nominate && idx->d_vectors_bf16 != nullptr && !vg::hook(vg::kHookFlatNoDma);
    const float eps_extra = bf16 ? vg::bf16_filter_eps(dot) : 0.0f;
    // ~want rows pass the sample threshold: the sel_k-th best of every sample_stride-th 128-row tile passes ~sel_k * sample_stride
    // (the select kernels hold 64 keys: beyond 4096 rows the stride grows).  The bf16 proof's margin is ~2^-7 (|q|^2 + max|x|^2):
    // the sample threshold sits further from the max_results-th score.  The list holds 2x and more of what is expected to pass.
    const int64_t want = std::max<int64_t>(static_cast<int64_t>(bf16 ? 3 : 2) * max_results, 512);
    const int sel_k = static_cast<int>(std::min<int64_t>(64, std::max<int64_t>(8, want / 64)));
    const int sample_stride = static_cast<int>(std::max<int64_t>(64, (want + 63) / 64));
    int cap = 4096;  // appended rows per query
    while (cap < (bf16 ? 6 : 3) * max_results) cap <<= 1;
    int64_t qc = std::min<int64_t>(4096, std::max<int64_t>(128, (int64_t(1) << 25) / cap));  // whole 128-query tiles, <= 2^25 keys
    qc = std::min<int64_t>(qc, nq);
    if (!nominate) qc = 0;
    const vg::ThrNomPlan plan{cap, sel_k, sample_stride, bf16, eps_extra};

    vg::ArenaCall ar(idx->ctx, st);
    const int i_lists = ar.add(sizeof(uint64_t) * static_cast<size_t>(vg::kThrQB) * list_cap);
    const int i_cnt = ar.add(sizeof(int) * vg::kThrQB);
    const size_t uqc = static_cast<size_t>(qc);
    const int i_nom = ar.add(vg::flat_thr_nominate_scratch(idx, plan, qc));
    const int i_fail = ar.add(sizeof(int) * (uqc + 1));
    const int i_todo = ar.add(sizeof(int) * (uqc + 1));
    const int i_elist = ar.add(sizeof(uint64_t) * uqc * cap);
    const int i_ecount = ar.add(sizeof(int) * uqc);
    VG_TRY(ar.commit());
    uint64_t *lists = ar.get<uint64_t>(i_lists);
    int *cnt = ar.get<int>(i_cnt);

    // one pass over the rows per kThrQB queries; qmap: the queries of the pass (device, null: the first cnt ones)
    auto scan = [&](const float *qp, const float *tp, const uint8_t *m0, const int *qmap, int c, uint32_t *oi, float *os,
                    int32_t *oc) -> int32_t {
        VG_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * vg::kThrQB, st));
        if (n > 0) {
            vg::ProfScope prof(idx->ctx, "flat_thr_scan", st);
            VG_TRY(vg::launch_thr_scan_f32(idx, qp, tp, qmap, c, m0, mask_stride, list_cap, lists, cnt, st));
        }
        vg::ProfScope prof(idx->ctx, "flat_thr_select", st);
        return vg::launch_thr_select_lists(dot, lists, list_cap, cnt, qmap, c, list_cap, max_results, oi, os, oc, st);
    };
    if (!nominate) {
        for (int64_t q0 = 0; q0 < nq; q0 += vg::kThrQB) {
            const int c = static_cast<int>(std::min<int64_t>(vg::kThrQB, nq - q0));
            VG_TRY(scan(io.q.ptr + q0 * dim, io.t.ptr + q0, io.mk.ptr ? io.mk.ptr + q0 * mask_stride : nullptr, nullptr, c,
                        io.oid.ptr + q0 * max_results, io.osc.ptr + q0 * max_results, io.ocnt.ptr + q0));
        }
        // (as vg_search_flat's small-batch scan: queries searched; VG_FLAT_FORCE_EXACT counts them as the exhaustive kernel's)
        if (idx->d_flat_stats)
            VG_LAUNCH(vg::flat_thr_stats_kernel, dim3(1), dim3(64), 0, st, idx->d_flat_stats, static_cast<long long>(nq),
                      static_cast<long long>(force_exact ? nq : 0));
    } else {
        uint64_t *elist = ar.get<uint64_t>(i_elist);
        vg::ThrNominated nom;
        int *fail = ar.get<int>(i_fail), *todo = ar.get<int>(i_todo), *ecount = ar.get<int>(i_ecount);
        int *always = fail + qc;  // (flat_todo_kernel's "every query" switch: off)
        VG_HIP(hipMemsetAsync(always, 0, sizeof(int), st));
        for (int64_t q0 = 0; q0 < nq; q0 += qc) {
            const int64_t c = std::min(qc, nq - q0);
            const float *qp = io.q.ptr + q0 * dim, *tp = io.t.ptr + q0;
            const uint8_t *m0 = io.mk.ptr ? io.mk.ptr + q0 * mask_stride : nullptr;
            uint32_t *oi = io.oid.ptr + q0 * max_results;
            float *os = io.osc.ptr + q0 * max_results;
            int32_t *oc = io.ocnt.ptr + q0;
            // (a) every row below the query's append threshold (the user's, widened, or the sample's) is appended
            VG_TRY(vg::flat_thr_nominate(idx, plan, qp, tp, c, m0, mask_stride, ar.get<char>(i_nom), &nom, st));
            // (b) re-scored exactly; the rows within the user's threshold form the query's list; (c) its best max_results
            {
                vg::ProfScope prof(idx->ctx, "flat_thr_rescore", st);
                VG_TRY(vg::launch_thr_rescore(dot, idx->d_vectors, dim, qp, tp, nom.cand, nom.counts, nullptr, c, cap, elist, ecount, st));
            }
            {
                vg::ProfScope prof(idx->ctx, "flat_thr_select", st);
                VG_TRY(vg::launch_thr_select_lists(dot, elist, cap, ecount, nullptr, c, cap, max_results, oi, os, oc, st));
            }
            // (d) the proof; the queries it leaves go to the scan, kThrQB per pass over the rows
            VG_TRY(vg::with_metric(dot, [&](auto dot_c) -> int32_t {
                VG_LAUNCH(vg::flat_thr_proof_kernel<decltype(dot_c)::value>, dim3(static_cast<unsigned>((c + 255) / 256)), dim3(256), 0, st, c,
                          nom.untight, nom.counts, cap, nom.gthr, nom.qnorm, idx->d_norm_max, dim, eps_extra, max_results, oc, os, fail);
                return VG_OK;
            }));
            VG_TRY(vg::launch_flat_todo(fail, always, static_cast<int>(c), todo, idx->d_flat_stats, st));
            int ntodo = 0;
            VG_HIP(hipMemcpyAsync(&ntodo, todo, sizeof(int), hipMemcpyDeviceToHost, st));
            VG_HIP(hipStreamSynchronize(st));
            for (int g = 0; g < ntodo; g += vg::kThrQB)
                VG_TRY(scan(qp, tp, m0, todo + 1 + g, std::min(vg::kThrQB, ntodo - g), oi, os, oc));
        }
    }
    // queries whose scores may hold a NaN: flat.Segment.Search(q, max_results) as its heap answers it, then the filter
    if (n > 0) {
        VG_TRY(vg::launch_cand_replay(vg::FlatF32Scorer{idx->d_vectors, idx->d_norm_max + 1, dim, dot, 0}, io.q.ptr, dim, n, nq,
                                      max_results, dot, io.mk.ptr, mask_stride, io.oid.ptr, io.osc.ptr, st));
        if (!vg::hook(vg::kHookNoCandReplay))
            VG_TRY(vg::launch_thr_filter(dot, io.t.ptr, nq, max_results, io.oid.ptr, io.osc.ptr, io.ocnt.ptr, st));
    }
    return io.finish();
}
