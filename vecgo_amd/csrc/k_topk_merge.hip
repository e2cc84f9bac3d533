// k_topk_merge.hip — the top-k fan-in merge for gfx950: per query the k best of several ascending key lists.  Every search family
// merges its per-slice lists through launch_topk_merge (vg_search.hpp); vg_merge_topk / vg_merge_topk_packed are the engine's
// fan-in over segments' (id, score) lists (engine/search.go:904-918), with the heap replay for lists that hold a NaN or a -0.0.
#include "vg_cand_replay.hpp"
#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"

namespace vg {

// One workgroup per query: merges `lists` ascending key lists of length k (kKeyMax padded)
// into the k best keys, best first, and decodes them to (id, score).
// Pruning: the k-th key of any single list bounds the global k-th key from above, and so does
// the k-th smallest list head; only keys <= T = min of the two bounds can make the result.
__global__ __launch_bounds__(kMergeThreads) void topk_merge_kernel(
    const uint64_t *__restrict__ partial, int lists, int k, bool descending,
    uint32_t *__restrict__ ids, float *__restrict__ scores, const int *__restrict__ only_if,
    const int *__restrict__ always)
{
    __shared__ uint64_t buf[kMergeBuf];
    __shared__ unsigned long long tmin;
    __shared__ int cnt;
    const int q = blockIdx.x;
    if (only_if && !only_if[q] && !(always && always[0])) return;  // query not selected
    const int tid = threadIdx.x;
    const uint64_t *src = partial + static_cast<int64_t>(q) * lists * k;
    const int64_t total = static_cast<int64_t>(lists) * k;
    uint32_t *oid = ids + static_cast<int64_t>(q) * k;
    float *osc = scores + static_cast<int64_t>(q) * k;
    if (tid == 0) {
        tmin = kKeyMax;
        cnt = 0;
    }
    __syncthreads();
    uint64_t t = kKeyMax;
    for (int l = tid; l < lists; l += kMergeThreads) {
        uint64_t v = src[static_cast<int64_t>(l) * k + (k - 1)];
        t = v < t ? v : t;
    }
    if (t != kKeyMax) atomicMin(&tmin, static_cast<unsigned long long>(t));
    // Second bound: the heads of k different lists are k different keys, so the k-th smallest HEAD
    // is >= the global k-th key too.  With many short lists it is far tighter than the first
    // (1024 lists of 10: ~2.5 survivors per list under T1, ~1.5k in total under the head bound).
    if (lists >= k && lists <= kMergeBuf && k >= 1) {
        int n2 = 1;
        while (n2 < lists) n2 <<= 1;
        for (int l = tid; l < n2; l += kMergeThreads) buf[l] = l < lists ? src[static_cast<int64_t>(l) * k] : kKeyMax;
        __syncthreads();
        bitonic_sort_lds(buf, n2, tid, kMergeThreads);
        const uint64_t hk = buf[k - 1];
        __syncthreads();  // everyone has read buf[k-1] before the buffer is reused below
        if (tid == 0 && hk != kKeyMax) atomicMin(&tmin, static_cast<unsigned long long>(hk));
    }
    __syncthreads();
    const uint64_t T = tmin;
    // lists are ascending: walk each from its head while keys stay <= T (usually 0-2 steps)
    for (int l = tid; l < lists; l += kMergeThreads) {
        const uint64_t *lp = src + static_cast<int64_t>(l) * k;
        for (int i = 0; i < k; i++) {
            const uint64_t key = lp[i];
            if (key == kKeyMax || key > T) break;
            int pos = atomicAdd(&cnt, 1);
            if (pos < kMergeBuf) buf[pos] = key;
        }
    }
    __syncthreads();
    const int c = cnt;
    int have;
    if (c <= 1024) {
        // brute-force rank among the survivors; a candidate listed twice (the same score and global id in two lists) is two
        // equal keys: the buffer position breaks the tie, so they take consecutive ranks, as the sort below places them
        for (int i = tid; i < c; i += kMergeThreads) {
            const uint64_t e = buf[i];
            int rank = 0;
            for (int j = 0; j < c; j++) {
                const uint64_t o = buf[j];
                rank += (o < e || (o == e && j < i)) ? 1 : 0;
            }
            if (rank < k) {
                oid[rank] = key_row(e);
                osc[rank] = key_score(e, descending);
            }
        }
        have = c < k ? c : k;
    } else {
        // many survivors (heavy ties / adversarial order): chunked sort of everything
        int kept = 0;
        int64_t pos = 0;
        __syncthreads();
        do {
            int room = kMergeBuf - kept;
            int take = static_cast<int>((total - pos) < room ? (total - pos) : room);
            for (int i = tid; i < take; i += kMergeThreads) buf[kept + i] = src[pos + i];
            for (int i = kept + take + tid; i < kMergeBuf; i += kMergeThreads) buf[i] = kKeyMax;
            __syncthreads();
            bitonic_sort_lds(buf, kMergeBuf, tid, kMergeThreads);
            pos += take;
            kept = k;  // k <= kAdcMaxK < kMergeBuf; slots past the real keys hold kKeyMax
        } while (pos < total);
        have = 0;
        for (int i = tid; i < k; i += kMergeThreads) {
            const uint64_t e = buf[i];
            if (e != kKeyMax) {
                oid[i] = key_row(e);
                osc[i] = key_score(e, descending);
            }
        }
        // count real keys among the first k (uniform across threads)
        int lo = 0, hi = k;
        while (lo < hi) {
            int mid = (lo + hi) >> 1;
            if (buf[mid] != kKeyMax) lo = mid + 1; else hi = mid;
        }
        have = lo;
    }
    for (int i = have + tid; i < k; i += kMergeThreads) {
        oid[i] = VG_INVALID_ID;
        osc[i] = descending ? -INFINITY : INFINITY;
    }
}

int32_t launch_topk_merge(const uint64_t *partial, int64_t nq, int lists, int k, bool descending,
                          uint32_t *ids, float *scores, hipStream_t st, const int *only_if, const int *always)
{
    if (nq == 0 || k == 0) return VG_OK;
    VG_LAUNCH(topk_merge_kernel, dim3(static_cast<unsigned>(nq)), dim3(kMergeThreads), 0,
                       st, partial, lists, k, descending, ids, scores, only_if, always);
    return VG_OK;
}

// (id, score) lists [lists][nq][k] -> keys [nq][lists][k] (ascending per list is preserved)
// list_stride: elements between the starts of two lists in ids[] / scores[] (nq*k when the lists are dense;
// 2*nq*k for the all-gathered [list][ids | score bits][nq][k] image of vg_comm.hip)
__global__ void pack_keys_kernel(const uint32_t *__restrict__ ids, const float *__restrict__ scores,
                                 int lists, int64_t nq, int k, int64_t list_stride, bool descending,
                                 const uint32_t *__restrict__ offsets, uint64_t *__restrict__ keys)
{
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t total = static_cast<int64_t>(lists) * nq * k;
    if (gid >= total) return;
    const int i = static_cast<int>(gid % k);
    const int64_t q = (gid / k) % nq;
    const int l = static_cast<int>(gid / (static_cast<int64_t>(k) * nq));
    const int64_t src = l * list_stride + q * k + i;
    const uint32_t id = ids[src];
    uint64_t key = kKeyMax;
    if (id != VG_INVALID_ID) key = make_key(scores[src], id + (offsets ? offsets[l] : 0u), descending);
    keys[(q * lists + l) * k + i] = key;
}

// The engine's fan-in when a list holds a NaN score (include/vecgo_hip.h "NaN scores"): engine/search.go:904-908 pushes every
// segment's candidates — in the order they were popped from the segment's heap, worst first, i.e. each list here from its last
// valid entry to its first — into ONE CandidateHeap with TryPushBounded(k), then pops it (:915-918).  The key merge above is that
// outcome while no score is a NaN; a query with one is replayed here by one wave and overwrites the key merge's answer.  Ids are
// the offset (global) ones: offsets ascend with the segment, so (SegmentID, RowID) orders like the global id.
__global__ __launch_bounds__(64) void merge_nan_replay_kernel(const uint32_t *__restrict__ ids_in, const float *__restrict__ scores_in, int lists,
                                                              int64_t nq, int k, int64_t list_stride, bool desc,
                                                              const uint32_t *__restrict__ offsets, uint32_t *__restrict__ ids,
                                                              float *__restrict__ scores)
{
    extern __shared__ uint64_t merge_lds[];
    CItem *heap = reinterpret_cast<CItem *>(merge_lds);
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    // a NaN, or a -0.0 score: InternalCandidateBetter compares floats, for which -0.0 == +0.0 (the lower global id wins),
    // while the key orders -0.0 strictly first; the replay below compares floats.  (The library's own searches emit one sign of
    // zero per metric; a caller's lists may hold both.)
    bool nan = false;
    for (int t = lane; t < lists * k; t += 64) {
        const int64_t src = static_cast<int64_t>(t / k) * list_stride + q * k + t % k;
        if (ids_in[src] != VG_INVALID_ID) {
            const float v = scores_in[src];
            nan = nan || v != v || __float_as_uint(v) == 0x80000000u;
        }
    }
    if (!__any(nan)) return;
    int len = 0;
    for (int l = 0; l < lists; l++) {
        const int64_t base = static_cast<int64_t>(l) * list_stride + q * k;
        int cnt = 0;  // valid entries are a prefix of the list
        for (int i0 = 0; i0 < k; i0 += 64) {
            const bool valid = i0 + lane < k && ids_in[base + i0 + lane] != VG_INVALID_ID;
            cnt += __popcll(__ballot(valid));
        }
        const uint32_t off = offsets ? offsets[l] : 0u;
        for (int i = cnt - 1; i >= 0; i--) {
            const CItem x{scores_in[base + i], ids_in[base + i] + off};
            if (len < k) {
                cand_up(heap, len, x, desc);
                len++;
            } else if (cand_better(x, cand_load(heap, 0), desc)) {
                cand_down(heap, 0, len, x, desc);
            }
        }
    }
    const int nres = len;
    for (int i = nres - 1; i >= 0; i--) {
        const CItem it = cand_pop(heap, len, desc);
        if (lane == 0) {
            ids[q * k + i] = it.row;
            scores[q * k + i] = it.score;
        }
    }
    for (int i = nres + lane; i < k; i += 64) {
        ids[q * k + i] = VG_INVALID_ID;
        scores[q * k + i] = desc ? -INFINITY : INFINITY;
    }
}
}  // namespace vg

static int32_t merge_topk_impl(vg_ctx *ctx, const uint32_t *ids_in, const float *scores_in, int64_t list_stride,
                               int32_t lists, int64_t nq, int32_t k, int32_t metric, const uint32_t *id_offsets,
                               uint32_t *ids, float *scores, void *stream);

VG_API int32_t vg_merge_topk(vg_ctx *ctx, const uint32_t *ids_in, const float *scores_in, int32_t lists,
                             int64_t nq, int32_t k, int32_t metric, const uint32_t *id_offsets,
                             uint32_t *ids, float *scores, void *stream)
{
    return merge_topk_impl(ctx, ids_in, scores_in, nq * k, lists, nq, k, metric, id_offsets, ids, scores, stream);
}

VG_API int32_t vg_merge_topk_packed(vg_ctx *ctx, const uint32_t *packed, int32_t lists, int64_t nq, int32_t k,
                                    int32_t metric, const uint32_t *id_offsets, uint32_t *ids, float *scores,
                                    void *stream)
{
    VG_CHECK(lists == 0 || nq == 0 || k == 0 || (packed && vg::is_device_ptr(packed)), VG_ERR_INVALID_ARG,
             "vg_merge_topk_packed: packed must be device memory");
    return merge_topk_impl(ctx, packed, reinterpret_cast<const float *>(packed) + nq * k, 2 * nq * k, lists, nq, k,
                           metric, id_offsets, ids, scores, stream);
}

static int32_t merge_topk_impl(vg_ctx *ctx, const uint32_t *ids_in, const float *scores_in, int64_t list_stride,
                               int32_t lists, int64_t nq, int32_t k, int32_t metric, const uint32_t *id_offsets,
                               uint32_t *ids, float *scores, void *stream)
{
    VG_CHECK(ctx, VG_ERR_INVALID_ARG, "vg_merge_topk: ctx is NULL");
    VG_CHECK(lists >= 0 && nq >= 0 && k >= 0, VG_ERR_INVALID_ARG, "vg_merge_topk: negative count");
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(ids && scores, VG_ERR_INVALID_ARG, "vg_merge_topk: NULL output");
    VG_CHECK(lists == 0 || (ids_in && scores_in), VG_ERR_INVALID_ARG, "vg_merge_topk: NULL input");
    VG_CHECK(k <= vg::kAdcMaxK, VG_ERR_UNSUPPORTED, "vg_merge_topk: k=%d exceeds %d", k, vg::kAdcMaxK);
    VG_CHECK(metric >= VG_METRIC_L2 && metric <= VG_METRIC_DOT, VG_ERR_UNSUPPORTED,
             "vg_merge_topk: unsupported metric %d", metric);
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = vg::pick_stream(ctx, stream);
    const bool desc = metric != VG_METRIC_L2;
    const size_t total = static_cast<size_t>(lists) * nq * k;
    const bool dense = list_stride == nq * k;  // the packed image is device memory already (checked by the caller)
    vg::DevIn<uint32_t> i_in, offs;
    vg::DevIn<float> s_in;
    vg::DevOut<uint32_t> oid;
    vg::DevOut<float> osc;
    if (dense) {
        VG_TRY(i_in.init(ids_in, total, st));
        VG_TRY(s_in.init(scores_in, total, st));
    } else {
        i_in.ptr = ids_in;
        s_in.ptr = scores_in;
    }
    VG_TRY(offs.init(id_offsets, id_offsets ? static_cast<size_t>(lists) : 0, st));
    VG_TRY(oid.init(ids, static_cast<size_t>(nq) * k, st));
    VG_TRY(osc.init(scores, static_cast<size_t>(nq) * k, st));
    const int nl = lists > 0 ? lists : 1;
    vg::ArenaCall ar(ctx, st);
    const int i_keys = ar.add(sizeof(uint64_t) * static_cast<size_t>(nl) * nq * k);
    VG_TRY(ar.commit());
    uint64_t *keys = ar.get<uint64_t>(i_keys);
    if (lists == 0) {
        VG_HIP(hipMemsetAsync(keys, 0xFF, static_cast<size_t>(nq) * k * 8, st));
    } else {
        VG_LAUNCH(vg::pack_keys_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256),
                           0, st, i_in.ptr, s_in.ptr, lists, nq, k, list_stride, desc, offs.ptr, keys);
    }
    VG_TRY(vg::launch_topk_merge(keys, nq, nl, k, desc, oid.ptr, osc.ptr, st));
    if (lists > 0 && !vg::hook(vg::kHookNoCandReplay))  // queries with a NaN or a -0.0 score in a list: the engine's heap, operation by operation
        VG_LAUNCH(vg::merge_nan_replay_kernel, dim3(static_cast<unsigned>(nq)), dim3(64), sizeof(uint64_t) * (static_cast<size_t>(k) + 4), st,
                  i_in.ptr, s_in.ptr, lists, nq, k, list_stride, desc, offs.ptr, oid.ptr, osc.ptr);
    VG_TRY(oid.finish());
    VG_TRY(osc.finish());
    return VG_OK;
}
