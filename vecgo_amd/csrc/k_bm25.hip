// k_bm25.hip — the lexical leg of Engine.HybridSearch (internal/engine/engine.go:1538-1640) for a batch:
//
//   vg_bm25_create / _search   lexical/bm25 MemoryIndex.Search (bm25.go:282-381) over a resident CSR image of the inverted index
//   vg_rrf_fuse                the Reciprocal Rank Fusion of engine.go:1560-1602
//
// The score.  The reference walks document at a time and adds a doc's terms in the query's term order, in float64, nothing
// fused.  That order is the binding constraint: no atomics across terms.  So the grid is (doc tile, query): a workgroup owns
// kTile consecutive docs, their float64 sums live in LDS (8192 docs = 64 KiB: two workgroups per CU); for each query term IN
// ORDER it walks the tile's sub-range of the term's ascending list (found by a 64-way search, a wave per term) with all lanes — a list names
// a doc once, so no two lanes touch the same sum — and a barrier separates the terms.  Then the docs with a sum > 0 are
// appended as keys (float32 score bits, doc id) to the query's list, and launch_thr_select_lists (k_flat_threshold.hip) takes
// the best k of every list.
//
// Ties.  candidateHeap (bm25.go:394-441) compares scores only, so among equal scores its LAYOUT decides what stays and in
// which order it pops.  The key selection is the heap's answer exactly when the best k scores are pairwise different and no
// further doc shares the k-th score (then the heap holds precisely the top k and pops them sorted).  bm25_risk_kernel tests
// that on the selection's output and the list; every other query is replayed: bm25_replay_kernel scores tile after tile with
// the same accumulate function and wave 0 runs the reference's push / up / down / pop on an LDS array over the docs in ascending
// order (64 docs are tested against the root per ballot, accepted ones applied one by one, as cand_replay_kernel does).
#include <algorithm>
#include <vector>

#include "vg_bm25.hpp"
#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"

namespace vg {
namespace {

constexpr int kTile = VG_BM25_TILE_DOCS;  // docs of one workgroup of the score kernel: their float64 sums fill 64 KiB of LDS
constexpr int kThreads = 512;
constexpr int kReplayTile = 2048;         // docs per step of the replay beside a large heap: 16 KiB + up to 16384 items (128 KiB)
constexpr int kUnroll = 4;               // postings a thread of the walk has in flight
constexpr int kMaxTerms = 64;             // terms of one query
constexpr int kRrfMax = 16384;            // entries of one query's two lists: 128 KiB of keys
constexpr int kRrfThreads = 1024;
static_assert(kTile * sizeof(double) == 65536, "the tile's sums are one 64 KiB LDS block");

struct Bm25Dev {
    const int64_t *term_off;
    const uint32_t *post_doc, *post_tf, *doc_len, *doc_to_id;
    int64_t n_terms;
    uint32_t n_docs;
    double k1_plus_1, k1_1b, k1_b_avgdl;
};

// the first of the ascending a[lo .. hi) that is >= key, by one wave: 64 probes per step (four dependent loads for a million
// postings where a binary search takes twenty)
__device__ __forceinline__ int64_t wave_lower_bound(const uint32_t *__restrict__ a, int64_t lo, int64_t hi, uint32_t key, int lane)
{
    for (;;) {
        const int64_t n = hi - lo;
        if (n <= 64) {
            const int64_t p = lo + lane;
            return lo + __popcll(__ballot(p < hi && a[p] < key));
        }
        const int64_t step = (n + 63) >> 6, probe = lo + (lane + 1) * step - 1;
        const int c = __popcll(__ballot(probe < hi && a[probe] < key));  // (ascending: the probes below the key are a prefix)
        const int64_t next_hi = lo + (c + 1) * step - 1;                 // the first probe that is not below the key, if there is one
        lo += c * step;
        if (next_hi < hi) hi = next_hi;
    }
}

// acc[i] <- the reference's score of doc d0 + i for i < nd, by the whole workgroup: the query's terms in order, a barrier
// between them.  Begins and ends with a barrier.  pos (LDS, one slot per term): the posting each term's walk of this tile
// begins at.  advance false: found here, a wave per term; true (the replay, which visits the tiles in ascending order and
// starts pos at every list's first posting): where the previous tile's walk ended, moved on past this tile's.
__device__ __forceinline__ void bm25_accumulate_tile(const Bm25Dev &ix, const uint32_t *__restrict__ terms, const double *__restrict__ idf,
                                                     int nt, uint32_t d0, uint32_t nd, double *acc, int tid, int nthreads,
                                                     unsigned long long *pos, bool advance)
{
    __syncthreads();  // the previous tile's sums have been read
    for (uint32_t i = tid; i < nd; i += nthreads) acc[i] = 0.0;
    if (!advance) {
        for (int t = tid >> 6; t < nt; t += nthreads >> 6) {
            const uint32_t term = terms[t];
            if (static_cast<int64_t>(term) >= ix.n_terms) continue;
            const int64_t lo = wave_lower_bound(ix.post_doc, ix.term_off[term], ix.term_off[term + 1], d0, tid & 63);
            if ((tid & 63) == 0) pos[t] = static_cast<unsigned long long>(lo);
        }
    }
    __syncthreads();
    for (int t = 0; t < nt; t++) {
        const uint32_t term = terms[t];
        if (static_cast<int64_t>(term) >= ix.n_terms) continue;  // a term the dictionary does not have: an empty list (bm25.go:302)
        const int64_t b = ix.term_off[term + 1], lo = static_cast<int64_t>(pos[t]);
        const double w = idf[t];
        unsigned mine = 0;  // postings of the tile this thread took
        // kUnroll postings per thread and step, their loads issued together: the chain posting -> doc length -> sum is the
        // walk's latency, and a workgroup this heavy in LDS has few neighbours to hide it
        for (int64_t p = lo + tid; p < b; p += static_cast<int64_t>(kUnroll) * nthreads) {
            uint32_t d[kUnroll], tfs[kUnroll], len[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const int64_t pu = p + static_cast<int64_t>(u) * nthreads;
                d[u] = pu < b ? ix.post_doc[pu] : 0xFFFFFFFFu;  // (no doc has this id: docs < 2^31)
            }
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const int64_t pu = p + static_cast<int64_t>(u) * nthreads;
                const bool in = d[u] - d0 < nd;
                tfs[u] = in ? ix.post_tf[pu] : 0u;
                len[u] = in ? ix.doc_len[d[u]] : 0u;
                mine += (in || d[u] < d0) ? 1u : 0u;  // (below the tile: an unsorted device-side list; skipped, never outside the tile's sums)
            }
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const uint32_t r = d[u] - d0;
                if (r >= nd) continue;
                const double tf = static_cast<double>(tfs[u]);
                const double doc_len = static_cast<double>(len[u]);
                const double num = tf * ix.k1_plus_1;
                const double denom = tf + ix.k1_1b + ix.k1_b_avgdl * doc_len;
                acc[r] = acc[r] + w * (num / denom);
            }
            if (d[0] >= d0 && d[0] - d0 >= nd) break;  // this thread's next postings lie past the tile too
        }
        if (advance) {  // every thread has read pos[t]; the barrier below separates this add from the next tile's read
            __syncthreads();
            if (mine) atomicAdd(&pos[t], static_cast<unsigned long long>(mine));
        }
        __syncthreads();
    }
}

// grid (doc tiles, queries of the chunk): the keys of the tile's docs with a score > 0, appended to the query's list
__global__ __launch_bounds__(kThreads) void bm25_score_kernel(Bm25Dev ix, const int32_t *__restrict__ q_off, const uint32_t *__restrict__ q_terms,
                                                              const double *__restrict__ q_idf, uint64_t *__restrict__ keys, int64_t key_cap,
                                                              int *__restrict__ counts)
{
    extern __shared__ double bm25_acc[];
    __shared__ unsigned long long pos[kMaxTerms];
    const int64_t q = blockIdx.y;
    const int t0 = q_off[q], nt = min(q_off[q + 1] - t0, kMaxTerms);
    if (nt <= 0) return;
    const uint32_t d0 = blockIdx.x * static_cast<uint32_t>(kTile);
    const uint32_t nd = min(static_cast<uint32_t>(kTile), ix.n_docs - d0);
    const int tid = threadIdx.x, lane = tid & 63;
    bm25_accumulate_tile(ix, q_terms + t0, q_idf + t0, nt, d0, nd, bm25_acc, tid, kThreads, pos, false);
    // the tile's hits: counted, one atomic for the workgroup (a query's tiles share one counter), then written
    __shared__ int wsum[kThreads / 64 + 1];
    const int wave = tid >> 6;
    int hits = 0;
    for (uint32_t i0 = 0; i0 < nd; i0 += kThreads) {
        const uint32_t i = i0 + tid;
        hits += __popcll(__ballot(i < nd && bm25_acc[i] > 0.0));  // bm25.go:363
    }
    if (lane == 0) wsum[wave] = hits;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < kThreads / 64; w++) total += wsum[w];
        wsum[kThreads / 64] = total ? atomicAdd(&counts[q], total) : 0;
    }
    __syncthreads();
    int64_t at = wsum[kThreads / 64];
    for (int w = 0; w < wave; w++) at += wsum[w];
    uint64_t *list = keys + q * key_cap;
    for (uint32_t i0 = 0; i0 < nd; i0 += kThreads) {
        const uint32_t i = i0 + tid;
        const double s = i < nd ? bm25_acc[i] : 0.0;
        const bool hit = s > 0.0;
        const uint64_t m = __ballot(hit);
        const int64_t mine = at + __popcll(m & ((uint64_t(1) << lane) - 1));
        if (hit && mine < key_cap) list[mine] = make_key(static_cast<float>(s), d0 + i, true);
        at += __popcll(m);
    }
}

// One workgroup per query of the chunk, after the selection: flag[q] <- must the heap be replayed?  (the best `kept` scores
// hold a tie, or another doc of the list shares the k-th score); the result's doc ids go through doc_to_id.
__global__ __launch_bounds__(256) void bm25_risk_kernel(const uint64_t *__restrict__ keys, int64_t key_cap, const int *__restrict__ counts, int k,
                                                        const uint32_t *__restrict__ doc_to_id, uint32_t *__restrict__ ids,
                                                        const float *__restrict__ scores, const int32_t *__restrict__ kept_of, int *__restrict__ flag)
{
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const int kept = kept_of[q];
    const int64_t hits = counts[q] < key_cap ? counts[q] : key_cap;
    const float *sc = scores + q * k;
    __shared__ int tie_s, same_s;
    if (tid == 0) tie_s = same_s = 0;
    __syncthreads();
    int tie = 0, same = 0;
    for (int i = 1 + tid; i < kept; i += 256) tie |= sc[i] == sc[i - 1];
    if (kept == k && hits > k) {  // the docs of the list with the k-th score: itself, and?
        const uint32_t kth = static_cast<uint32_t>(make_key(sc[k - 1], 0u, true) >> 32);
        for (int64_t i = tid; i < hits; i += 256) same += static_cast<uint32_t>(keys[q * key_cap + i] >> 32) == kth;
    }
    if (tie) tie_s = 1;  // (the same value from every writer)
    if (same) atomicAdd(&same_s, same);
    __syncthreads();
    if (tid == 0) flag[q] = tie_s || same_s >= 2;
    if (doc_to_id)
        for (int i = tid; i < kept; i += 256) ids[q * k + i] = doc_to_id[ids[q * k + i]];
}

struct Bm25Item {
    float score;
    uint32_t id;
};
// candidateHeap (bm25.go:394-441): a binary min-heap by score alone
__device__ __forceinline__ void bm25_up(Bm25Item *h, int j)
{
    for (;;) {
        const int i = (j - 1) / 2;  // (Go's division truncates: the root is its own parent)
        if (i == j || h[j].score >= h[i].score) break;
        const Bm25Item x = h[i];
        h[i] = h[j];
        h[j] = x;
        j = i;
    }
}
__device__ __forceinline__ void bm25_down(Bm25Item *h, int i, int n)
{
    for (;;) {
        const int j1 = 2 * i + 1;
        if (j1 >= n) break;
        int j = j1;
        if (j1 + 1 < n && h[j1 + 1].score < h[j1].score) j = j1 + 1;
        if (h[j].score >= h[i].score) break;
        const Bm25Item x = h[i];
        h[i] = h[j];
        h[j] = x;
        i = j;
    }
}

// One workgroup per query; a query without its flag returns at once.  Overwrites what the selection wrote for the query.
__global__ __launch_bounds__(kThreads) void bm25_replay_kernel(Bm25Dev ix, const int32_t *__restrict__ q_off, const uint32_t *__restrict__ q_terms,
                                                               const double *__restrict__ q_idf, const int *__restrict__ flag, int k,
                                                               uint32_t *__restrict__ ids, float *__restrict__ scores, int32_t *__restrict__ out_counts,
                                                               unsigned long long *__restrict__ replayed, uint32_t tile)
{
    extern __shared__ double bm25_acc[];  // `tile` sums, then the heap's k items
    __shared__ unsigned long long cursor[kMaxTerms];
    Bm25Item *heap = reinterpret_cast<Bm25Item *>(bm25_acc + tile);
    const int64_t q = blockIdx.x;
    if (!flag[q]) return;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) atomicAdd(replayed, 1ull);
    const int t0 = q_off[q], nt = min(q_off[q + 1] - t0, kMaxTerms);
    if (tid < nt) {
        const uint32_t term = q_terms[t0 + tid];
        cursor[tid] = static_cast<int64_t>(term) < ix.n_terms ? static_cast<unsigned long long>(ix.term_off[term]) : 0ull;
    }
    int len = 0;  // wave 0's copy is the live one
    for (uint32_t d0 = 0; d0 < ix.n_docs; d0 += tile) {
        const uint32_t nd = min(tile, ix.n_docs - d0);
        bm25_accumulate_tile(ix, q_terms + t0, q_idf + t0, nt, d0, nd, bm25_acc, tid, kThreads, cursor, true);
        if (tid >= 64) continue;
        for (uint32_t j0 = 0; j0 < nd; j0 += 64) {
            const uint32_t j = j0 + lane;
            const double s = j < nd ? bm25_acc[j] : 0.0;
            const bool live = s > 0.0;
            const float mine = static_cast<float>(s);
            int from = 0;  // lanes below it have been decided
            for (;;) {
                // bm25.go:365-370 against the heap as it stands: a lane that fails now is tested again after every accepted doc
                const float root = len > 0 ? heap[0].score : 0.0f;
                const uint64_t m = __ballot(live && lane >= from && (len < k || mine > root));
                if (m == 0) break;
                const int b = __builtin_ctzll(m);
                const uint32_t d = d0 + j0 + static_cast<uint32_t>(b);
                const Bm25Item x{__uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(mine), b)), ix.doc_to_id ? ix.doc_to_id[d] : d};
                if (len < k) {  // h.push
                    heap[len] = x;
                    bm25_up(heap, len);
                    len++;
                } else {
                    heap[0] = x;
                    bm25_down(heap, 0, len);
                }
                from = b + 1;
            }
        }
    }
    if (tid >= 64) return;
    const int nres = len;
    for (int i = nres - 1; i >= 0; i--) {  // candidates[i] = h.pop()
        const Bm25Item root = heap[0];
        heap[0] = heap[len - 1];
        len--;
        if (len > 0) bm25_down(heap, 0, len);
        if (lane == 0) {
            ids[q * k + i] = root.id;
            scores[q * k + i] = root.score;
        }
    }
    for (int i = nres + lane; i < k; i += 64) {
        ids[q * k + i] = VG_INVALID_ID;
        scores[q * k + i] = -INFINITY;
    }
    if (lane == 0) out_counts[q] = nres;
}

// ---- Reciprocal Rank Fusion ---------------------------------------------------------------------------------------------
// One workgroup per query.  The entries of both lists as keys (id, source, rank) are sorted in LDS; the first key of every id
// walks its group — list A's ranks ascending, then list B's — as the reference's two loops meet the id: A sets, the last rank
// staying (engine.go:1568-1571), B adds in ascending rank (:1574-1577).  The fused (score, id) keys are sorted again: score
// descending, id ascending among equal scores.
__global__ __launch_bounds__(kRrfThreads) void rrf_fuse_kernel(const uint32_t *__restrict__ a_ids, const int32_t *__restrict__ a_counts, int64_t a_stride,
                                                               const uint32_t *__restrict__ b_ids, const int32_t *__restrict__ b_counts, int64_t b_stride,
                                                               int rrf_k, int k, uint32_t *__restrict__ out_ids, float *__restrict__ out_scores,
                                                               int32_t *__restrict__ out_counts)
{
    extern __shared__ uint64_t rrf_lds[];
    __shared__ int unique_s;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    int ca = a_ids && a_counts ? static_cast<int>(min(static_cast<int64_t>(max(a_counts[q], 0)), min(a_stride, static_cast<int64_t>(kRrfMax)))) : 0;
    int cb = b_ids && b_counts ? static_cast<int>(min(static_cast<int64_t>(max(b_counts[q], 0)), min(b_stride, static_cast<int64_t>(kRrfMax)))) : 0;
    if (ca + cb > kRrfMax) cb = kRrfMax - ca;  // (refused on the host where the host can see it)
    const int n = ca + cb;
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    if (tid == 0) unique_s = 0;
    for (int i = tid; i < n2; i += kRrfThreads) {
        uint64_t key = kKeyMax;
        if (i < n) {
            const bool from_b = i >= ca;
            const uint32_t rank = from_b ? i - ca : i;
            const uint32_t id = from_b ? b_ids[q * b_stride + rank] : a_ids[q * a_stride + rank];
            if (id != VG_INVALID_ID) key = (static_cast<uint64_t>(id) << 32) | (from_b ? 0x80000000u : 0u) | rank;
        }
        rrf_lds[i] = key;
    }
    __syncthreads();
    bitonic_sort_lds(rrf_lds, n2, tid, kRrfThreads);
    uint64_t fused[kRrfMax / kRrfThreads];
    int heads = 0;
#pragma unroll
    for (int s = 0; s < kRrfMax / kRrfThreads; s++) {
        const int i = s * kRrfThreads + tid;
        fused[s] = kKeyMax;
        if (i >= n2) continue;
        const uint64_t key = rrf_lds[i];
        if (key == kKeyMax) continue;
        const uint32_t id = static_cast<uint32_t>(key >> 32);
        if (i > 0 && static_cast<uint32_t>(rrf_lds[i - 1] >> 32) == id) continue;  // not the id's first key
        float score = 0.0f;  // finalScores[id] of an id list A does not hold
        for (int j = i; j < n2; j++) {
            const uint64_t e = rrf_lds[j];
            if (static_cast<uint32_t>(e >> 32) != id) break;
            const uint32_t low = static_cast<uint32_t>(e);
            const float term = __fdiv_rn(1.0f, static_cast<float>(static_cast<int64_t>(rrf_k) + (low & 0x7FFFFFFFu) + 1));
            score = (low >> 31) ? score + term : term;
        }
        fused[s] = make_key(score, id, true);
        heads++;
    }
    if (heads) atomicAdd(&unique_s, heads);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kRrfMax / kRrfThreads; s++) {
        const int i = s * kRrfThreads + tid;
        if (i < n2) rrf_lds[i] = fused[s];
    }
    __syncthreads();
    bitonic_sort_lds(rrf_lds, n2, tid, kRrfThreads);
    const int kept = unique_s < k ? unique_s : k;
    for (int i = tid; i < k; i += kRrfThreads) {
        const uint64_t e = i < kept ? rrf_lds[i] : kKeyMax;
        out_ids[q * k + i] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        out_scores[q * k + i] = e == kKeyMax ? -INFINITY : key_score(e, true);
    }
    if (tid == 0 && out_counts) out_counts[q] = kept;
}

// the answer of an index without docs (bm25.go:286): nothing, for every query
__global__ __launch_bounds__(256) void bm25_empty_answer_kernel(uint32_t *__restrict__ ids, float *__restrict__ scores, int32_t *__restrict__ counts,
                                                                int64_t nq, int k)
{
    const int64_t total = nq * k;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        ids[i] = VG_INVALID_ID;
        scores[i] = -INFINITY;
        if (counts && i < nq) counts[i] = 0;
    }
}

template <typename T>
int32_t upload(T **dst, const T *src, size_t count, hipStream_t st)
{
    VG_HIP(hipMalloc(reinterpret_cast<void **>(dst), std::max<size_t>(count, 1) * sizeof(T)));
    if (count) VG_HIP(hipMemcpyAsync(*dst, src, count * sizeof(T), is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    return VG_OK;
}

struct QueryChunk {
    int64_t q0, q1, longest;
};

}  // namespace
}  // namespace vg

void vg::bm25_set_constants(vg_bm25 *bm, int64_t total_length, int64_t doc_count)
{
    const double avg_dl = static_cast<double>(total_length) / static_cast<double>(doc_count);  // bm25.go:314-317; k1 = 1.2, b = 0.75
    bm->k1_plus_1 = 2.2;  // the reference's constants are exact constant expressions rounded ONCE: k1 + 1, k1 * (1 - b), k1 * b
    bm->k1_1b = 0.3;
    bm->k1_b_avgdl = 0.9 / avg_dl;
    bm->doc_count = doc_count;
}

VG_API int32_t vg_bm25_destroy(vg_bm25 *bm)
{
    if (!bm) return VG_OK;
    (void)hipSetDevice(bm->ctx->device);
    (void)hipDeviceSynchronize();  // a search on any stream may still read it
    vg::drop_device(&bm->d_term_off);
    vg::drop_device(&bm->d_post_doc);
    vg::drop_device(&bm->d_post_tf);
    vg::drop_device(&bm->d_doc_len);
    vg::drop_device(&bm->d_doc_to_id);
    vg::drop_device(&bm->d_alt_off);
    vg::drop_device(&bm->d_alt_doc);
    vg::drop_device(&bm->d_alt_tf);
    vg::drop_device(&bm->d_replayed);
    delete bm;
    return VG_OK;
}

VG_API int32_t vg_bm25_create(vg_ctx *ctx, int64_t n_docs, int64_t n_terms, const int64_t *term_off, const uint32_t *post_doc,
                              const uint32_t *post_tf, const uint32_t *doc_len, int64_t total_length, int64_t doc_count,
                              const uint32_t *doc_to_id, vg_bm25 **out)
{
    VG_CHECK(ctx && out, VG_ERR_INVALID_ARG, "vg_bm25_create: NULL context or result");
    *out = nullptr;
    VG_CHECK(n_docs >= 0 && n_terms >= 0, VG_ERR_INVALID_ARG, "vg_bm25_create: n_docs = %lld, n_terms = %lld: negative", (long long)n_docs,
             (long long)n_terms);
    VG_CHECK(n_docs < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "vg_bm25_create: %lld docs, fewer than 2^31 are supported", (long long)n_docs);
    VG_CHECK(n_terms < (int64_t(1) << 32) - 1, VG_ERR_UNSUPPORTED, "vg_bm25_create: %lld terms, term ids are uint32", (long long)n_terms);
    VG_CHECK(doc_count >= 1, VG_ERR_INVALID_ARG, "vg_bm25_create: doc_count = %lld, at least 1 (an index without docs answers nothing)",
             (long long)doc_count);
    VG_CHECK(total_length >= 0, VG_ERR_INVALID_ARG, "vg_bm25_create: total_length = %lld: negative", (long long)total_length);
    VG_CHECK(term_off, VG_ERR_INVALID_ARG, "vg_bm25_create: NULL term_off");
    VG_CHECK(doc_len || n_docs == 0, VG_ERR_INVALID_ARG, "vg_bm25_create: NULL doc_len");
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    std::vector<int64_t> h_off(static_cast<size_t>(n_terms) + 1);
    if (vg::is_device_ptr(term_off)) {
        VG_HIP(hipMemcpyAsync(h_off.data(), term_off, h_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        VG_HIP(hipStreamSynchronize(st));
    } else {
        std::copy(term_off, term_off + h_off.size(), h_off.begin());
    }
    VG_CHECK(h_off[0] == 0, VG_ERR_INVALID_ARG, "vg_bm25_create: term_off[0] = %lld, not 0", (long long)h_off[0]);
    for (int64_t t = 0; t < n_terms; t++)
        VG_CHECK(h_off[t + 1] >= h_off[t], VG_ERR_INVALID_ARG, "vg_bm25_create: term_off decreases at term %lld", (long long)t);
    const int64_t n_post = h_off[static_cast<size_t>(n_terms)];
    VG_CHECK(n_post >= 0 && static_cast<uint64_t>(n_post) < (uint64_t(1) << 63), VG_ERR_UNSUPPORTED,
             "vg_bm25_create: %lld postings, fewer than 2^63 are supported", (long long)n_post);
    VG_CHECK((post_doc && post_tf) || n_post == 0, VG_ERR_INVALID_ARG, "vg_bm25_create: NULL postings");
    if (n_post > 0 && !vg::is_device_ptr(post_doc)) {  // the lists the host can read: strictly ascending docs below n_docs
        for (int64_t t = 0; t < n_terms; t++)
            for (int64_t p = h_off[t]; p < h_off[t + 1]; p++) {
                VG_CHECK(static_cast<int64_t>(post_doc[p]) < n_docs, VG_ERR_INVALID_ARG, "vg_bm25_create: term %lld names doc %u of %lld",
                         (long long)t, post_doc[p], (long long)n_docs);
                VG_CHECK(p == h_off[t] || post_doc[p] > post_doc[p - 1], VG_ERR_INVALID_ARG,
                         "vg_bm25_create: the posting list of term %lld is not in strictly ascending doc order (doc %u after doc %u)",
                         (long long)t, post_doc[p], post_doc[p - 1]);
            }
    }

    vg_bm25 *bm = new vg_bm25();
    bm->ctx = ctx;
    bm->n_docs = n_docs;
    bm->n_terms = n_terms;
    bm->n_post = n_post;
    bm->mapped = doc_to_id != nullptr;
    vg::bm25_set_constants(bm, total_length, doc_count);
    int32_t s = vg::upload(&bm->d_term_off, h_off.data(), h_off.size(), st);
    if (s == VG_OK) s = vg::upload(&bm->d_post_doc, post_doc, static_cast<size_t>(n_post), st);
    if (s == VG_OK) s = vg::upload(&bm->d_post_tf, post_tf, static_cast<size_t>(n_post), st);
    if (s == VG_OK) s = vg::upload(&bm->d_doc_len, doc_len, static_cast<size_t>(n_docs), st);
    if (s == VG_OK && doc_to_id) s = vg::upload(&bm->d_doc_to_id, doc_to_id, static_cast<size_t>(n_docs), st);
    if (s == VG_OK) s = vg::upload<unsigned long long>(&bm->d_replayed, nullptr, 0, st);
    if (s == VG_OK && hipMemsetAsync(bm->d_replayed, 0, sizeof(unsigned long long), st) != hipSuccess) s = VG_ERR_HIP;
    if (s == VG_OK && hipStreamSynchronize(st) != hipSuccess) {
        vg::set_error("vg_bm25_create: the upload failed");
        s = VG_ERR_HIP;
    }
    if (s != VG_OK) {
        (void)vg_bm25_destroy(bm);
        return s;
    }
    bm->h_term_off = std::move(h_off);
    *out = bm;
    return VG_OK;
}

VG_API int32_t vg_bm25_stats(vg_bm25 *bm, int64_t *docs, int64_t *terms, int64_t *postings, int64_t *bytes)
{
    VG_CHECK(bm, VG_ERR_INVALID_ARG, "vg_bm25_stats: NULL index");
    if (docs) *docs = bm->n_docs;
    if (terms) *terms = bm->n_terms;
    if (postings) *postings = bm->n_post;
    if (bytes) {  // what is held: an array vg_bm25_update has grown counts with its room, and so does the second image
        const int64_t off = std::max(bm->off_cap, bm->n_terms + 1) + (bm->d_alt_off ? bm->alt_off_cap : 0);
        const int64_t post = std::max(bm->post_cap, bm->n_post) + (bm->d_alt_doc ? bm->alt_post_cap : 0);
        const int64_t docs = std::max(bm->docs_cap, bm->n_docs);
        *bytes = off * 8 + post * 8 + docs * 4 + (bm->d_doc_to_id ? docs * 4 : 0);
    }
    return VG_OK;
}

VG_API int32_t vg_bm25_replayed(vg_bm25 *bm, int64_t *replayed, void *stream)
{
    VG_CHECK(bm && replayed, VG_ERR_INVALID_ARG, "vg_bm25_replayed: NULL index or pointer");
    VG_HIP(hipSetDevice(bm->ctx->device));
    hipStream_t st = vg::pick_stream(bm->ctx, stream);
    unsigned long long v = 0;
    VG_HIP(hipMemcpyAsync(&v, bm->d_replayed, sizeof(v), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    *replayed = static_cast<int64_t>(v);
    return VG_OK;
}

VG_API int32_t vg_bm25_search(vg_bm25 *bm, const int32_t *q_term_off, const uint32_t *q_terms, const double *q_idf, int64_t nq, int32_t k,
                              uint32_t *out_ids, float *out_scores, int32_t *out_counts, void *stream)
{
    VG_CHECK(bm, VG_ERR_INVALID_ARG, "vg_bm25_search: NULL index");
    VG_CHECK(nq >= 0 && k >= 0, VG_ERR_INVALID_ARG, "vg_bm25_search: negative nq or k");
    VG_CHECK(k <= vg::kThrMaxResults, VG_ERR_UNSUPPORTED, "vg_bm25_search: k=%d exceeds %d", k, vg::kThrMaxResults);
    VG_CHECK(nq < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "vg_bm25_search: %lld queries, fewer than 2^31 are supported", (long long)nq);
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(q_term_off && out_ids && out_scores, VG_ERR_INVALID_ARG, "vg_bm25_search: NULL buffer");
    vg_ctx *ctx = bm->ctx;
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = vg::pick_stream(ctx, stream);

    // the query arrays on the host: their shape is checked, and the lists' lengths bound every query's hits
    std::vector<int32_t> off_store;
    std::vector<uint32_t> term_store;
    const int32_t *h_off = nullptr;
    const uint32_t *h_terms = nullptr;
    VG_TRY(vg::host_view(q_term_off, static_cast<size_t>(nq) + 1, st, off_store, h_off));
    VG_CHECK(h_off[0] >= 0, VG_ERR_INVALID_ARG, "vg_bm25_search: q_term_off[0] = %d: negative", h_off[0]);
    for (int64_t q = 0; q < nq; q++) {
        VG_CHECK(h_off[q + 1] >= h_off[q], VG_ERR_INVALID_ARG, "vg_bm25_search: q_term_off decreases at query %lld", (long long)q);
        VG_CHECK(h_off[q + 1] - h_off[q] <= vg::kMaxTerms, VG_ERR_UNSUPPORTED, "vg_bm25_search: query %lld has %d terms, at most %d are supported",
                 (long long)q, h_off[q + 1] - h_off[q], vg::kMaxTerms);
    }
    const size_t n_qterms = static_cast<size_t>(h_off[nq]);
    VG_CHECK((q_terms && q_idf) || n_qterms == 0, VG_ERR_INVALID_ARG, "vg_bm25_search: NULL q_terms or q_idf");
    VG_TRY(vg::host_view(q_terms, n_qterms, st, term_store, h_terms));
    std::vector<int64_t> bound(static_cast<size_t>(nq));
    for (int64_t q = 0; q < nq; q++) {
        int64_t sum = 0;
        for (int32_t t = h_off[q]; t < h_off[q + 1]; t++)
            if (static_cast<int64_t>(h_terms[t]) < bm->n_terms) sum += bm->h_term_off[h_terms[t] + 1] - bm->h_term_off[h_terms[t]];
        bound[q] = std::min(sum, bm->n_docs);
    }

    vg::DevIn<int32_t> d_off;
    vg::DevIn<uint32_t> d_terms;
    vg::DevIn<double> d_idf;
    vg::DevOut<uint32_t> oid;
    vg::DevOut<float> osc;
    vg::DevOut<int32_t> ocnt;
    vg::DevTmp<int32_t> own_cnt;
    VG_TRY(d_off.init(q_term_off, static_cast<size_t>(nq) + 1, st, vg::kAnyAlign));
    VG_TRY(d_terms.init(q_terms, n_qterms, st, vg::kAnyAlign));
    VG_TRY(d_idf.init(q_idf, n_qterms, st, vg::kAnyAlign));
    VG_TRY(oid.init(out_ids, static_cast<size_t>(nq) * k, st, vg::kAnyAlign));
    VG_TRY(osc.init(out_scores, static_cast<size_t>(nq) * k, st, vg::kAnyAlign));
    if (out_counts) {
        VG_TRY(ocnt.init(out_counts, static_cast<size_t>(nq), st, vg::kAnyAlign));
    } else {
        VG_TRY(own_cnt.init(static_cast<size_t>(nq), st));
    }
    int32_t *cnt_out = out_counts ? ocnt.ptr : own_cnt.ptr;
    if (bm->doc_count == 0) {  // bm25.go:286: an index without docs (vg_bm25_create_empty, or updated down to none) answers nothing
        const int64_t total = nq * k;
        VG_LAUNCH(vg::bm25_empty_answer_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((total + 255) / 256, 1024))), dim3(256), 0, st, oid.ptr,
                  osc.ptr, cnt_out, nq, k);
        VG_TRY(oid.finish());
        VG_TRY(osc.finish());
        if (out_counts) VG_TRY(ocnt.finish());
        if (d_off.owned || d_terms.owned || d_idf.owned) VG_HIP(hipStreamSynchronize(st));
        return VG_OK;
    }

    // query chunks whose key lists (8 bytes per query and slot of the chunk's longest list) stay inside the context's scratch cap
    const int64_t cap_bytes = vg::hook(vg::kHookBm25SmallScratch) ? 65536 : vg::scratch_cap(ctx);  // (the hook: several chunks for a test batch)
    std::vector<vg::QueryChunk> chunks;
    vg::QueryChunk c{0, 0, 0};
    for (int64_t q = 0; q < nq; q++) {
        int64_t longest = std::max(c.longest, bound[q]);
        if (q > c.q0 && ((q - c.q0 + 1) * std::max<int64_t>(longest, 1) * 8 > cap_bytes || q - c.q0 >= 65535)) {
            chunks.push_back(c);  // query q opens the next chunk
            c = vg::QueryChunk{q, q, 0};
            longest = bound[q];
        }
        c.q1 = q + 1;
        c.longest = longest;
    }
    chunks.push_back(c);
    size_t keys_bytes = 8;
    for (const vg::QueryChunk &ch : chunks)
        keys_bytes = std::max(keys_bytes, static_cast<size_t>(ch.q1 - ch.q0) * static_cast<size_t>(std::max<int64_t>(ch.longest, 1)) * sizeof(uint64_t));
    vg::ArenaCall ar(ctx, st);
    const int i_keys = ar.add(keys_bytes), i_cnt = ar.add(sizeof(int) * static_cast<size_t>(nq)), i_flag = ar.add(sizeof(int) * static_cast<size_t>(nq));
    VG_TRY(ar.commit());
    uint64_t *keys = ar.get<uint64_t>(i_keys);
    int *cnt = ar.get<int>(i_cnt), *flag = ar.get<int>(i_flag);
    VG_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * static_cast<size_t>(nq), st));

    const vg::Bm25Dev ix{bm->d_term_off, bm->d_post_doc, bm->d_post_tf, bm->d_doc_len, bm->d_doc_to_id, bm->n_terms,
                         static_cast<uint32_t>(bm->n_docs), bm->k1_plus_1, bm->k1_1b, bm->k1_b_avgdl};
    const unsigned tiles = static_cast<unsigned>((bm->n_docs + vg::kTile - 1) / vg::kTile);
    for (const vg::QueryChunk &ch : chunks) {
        const int64_t n = ch.q1 - ch.q0, key_cap = std::max<int64_t>(ch.longest, 1);
        if (ch.longest > 0) {
            vg::ProfScope prof(ctx, "bm25_score", st);
            // (64 KiB of sums and the terms' positions: above the default limit of a launch)
            VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vg::bm25_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(vg::kTile * sizeof(double) + 1024)));
            VG_LAUNCH(vg::bm25_score_kernel, dim3(tiles, static_cast<unsigned>(n)), dim3(vg::kThreads), vg::kTile * sizeof(double), st, ix,
                      d_off.ptr + ch.q0, d_terms.ptr, d_idf.ptr, keys, key_cap, cnt + ch.q0);
        }
        vg::ProfScope prof(ctx, "bm25_select", st);
        VG_TRY(vg::launch_thr_select_lists(true, keys, key_cap, cnt + ch.q0, nullptr, n, key_cap, k, oid.ptr + ch.q0 * k, osc.ptr + ch.q0 * k,
                                           cnt_out + ch.q0, st));
        VG_LAUNCH(vg::bm25_risk_kernel, dim3(static_cast<unsigned>(n)), dim3(256), 0, st, keys, key_cap, cnt + ch.q0, k, bm->d_doc_to_id,
                  oid.ptr + ch.q0 * k, osc.ptr + ch.q0 * k, cnt_out + ch.q0, flag + ch.q0);
    }
    if (bm->n_docs > 0) {  // the queries at risk: the reference's heap over the docs in ascending order
        vg::ProfScope prof(ctx, "bm25_replay", st);
        // the score kernel's tile where two workgroups of it and their heaps still share a CU's LDS, else a quarter of it
        const size_t heap_bytes = (static_cast<size_t>(k) + 1) * sizeof(vg::Bm25Item);
        const uint32_t tile = heap_bytes <= 8192 ? vg::kTile : vg::kReplayTile;
        const size_t lds = tile * sizeof(double) + heap_bytes;
        if (lds > 65536)
            VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vg::bm25_replay_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds + 1024)));
        VG_LAUNCH(vg::bm25_replay_kernel, dim3(static_cast<unsigned>(nq)), dim3(vg::kThreads), lds, st, ix, d_off.ptr, d_terms.ptr, d_idf.ptr, flag, k,
                  oid.ptr, osc.ptr, cnt_out, bm->d_replayed, tile);
    }
    VG_TRY(oid.finish());
    VG_TRY(osc.finish());
    if (out_counts) VG_TRY(ocnt.finish());
    if (d_off.owned || d_terms.owned || d_idf.owned) VG_HIP(hipStreamSynchronize(st));  // the caller's host arrays have been read
    return VG_OK;
}

VG_API int32_t vg_rrf_fuse(vg_ctx *ctx, int64_t nq, const uint32_t *a_ids, const int32_t *a_counts, int64_t a_stride, const uint32_t *b_ids,
                           const int32_t *b_counts, int64_t b_stride, int32_t rrf_k, int32_t k, uint32_t *out_ids, float *out_scores,
                           int32_t *out_counts, void *stream)
{
    VG_CHECK(ctx, VG_ERR_INVALID_ARG, "vg_rrf_fuse: NULL context");
    VG_CHECK(nq >= 0 && k >= 0 && a_stride >= 0 && b_stride >= 0 && rrf_k >= 0, VG_ERR_INVALID_ARG,
             "vg_rrf_fuse: nq = %lld, k = %d, a_stride = %lld, b_stride = %lld, rrf_k = %d: negative", (long long)nq, k, (long long)a_stride,
             (long long)b_stride, rrf_k);
    VG_CHECK(k <= vg::kRrfMax, VG_ERR_UNSUPPORTED, "vg_rrf_fuse: k=%d exceeds %d", k, vg::kRrfMax);
    VG_CHECK(nq < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "vg_rrf_fuse: %lld queries, fewer than 2^31 are supported", (long long)nq);
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(out_ids && out_scores, VG_ERR_INVALID_ARG, "vg_rrf_fuse: NULL output");
    const bool has_a = a_ids && a_counts && a_stride > 0, has_b = b_ids && b_counts && b_stride > 0;
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = vg::pick_stream(ctx, stream);
    // the limit, where the host can see the counts; device counts are cut to their stride, so the strides bound them
    const bool host_a = has_a && !vg::is_device_ptr(a_counts), host_b = has_b && !vg::is_device_ptr(b_counts);
    int64_t most = 0;
    {
        for (int64_t q = 0; q < nq; q++) {
            const int64_t ca = host_a ? std::min<int64_t>(std::max(a_counts[q], 0), a_stride) : 0;
            const int64_t cb = host_b ? std::min<int64_t>(std::max(b_counts[q], 0), b_stride) : 0;
            most = std::max(most, ca + cb);
        }
        if (has_a && !host_a) most += a_stride;
        if (has_b && !host_b) most += b_stride;
    }
    VG_CHECK(most <= vg::kRrfMax, VG_ERR_UNSUPPORTED, "vg_rrf_fuse: %lld entries in a query's two lists, at most %d are supported", (long long)most,
             vg::kRrfMax);
    vg::DevIn<uint32_t> da, db;
    vg::DevIn<int32_t> dca, dcb;
    vg::DevOut<uint32_t> oid;
    vg::DevOut<float> osc;
    vg::DevOut<int32_t> ocnt;
    if (has_a) {
        VG_TRY(da.init(a_ids, static_cast<size_t>(nq * a_stride), st, vg::kAnyAlign));
        VG_TRY(dca.init(a_counts, static_cast<size_t>(nq), st, vg::kAnyAlign));
    }
    if (has_b) {
        VG_TRY(db.init(b_ids, static_cast<size_t>(nq * b_stride), st, vg::kAnyAlign));
        VG_TRY(dcb.init(b_counts, static_cast<size_t>(nq), st, vg::kAnyAlign));
    }
    VG_TRY(oid.init(out_ids, static_cast<size_t>(nq) * k, st, vg::kAnyAlign));
    VG_TRY(osc.init(out_scores, static_cast<size_t>(nq) * k, st, vg::kAnyAlign));
    VG_TRY(ocnt.init(out_counts, out_counts ? static_cast<size_t>(nq) : 0, st, vg::kAnyAlign));
    int n2 = 2;
    while (n2 < most) n2 <<= 1;
    const size_t lds = static_cast<size_t>(n2) * sizeof(uint64_t);
    {
        vg::ProfScope prof(ctx, "rrf_fuse", st);
        if (lds > 65536)
            VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vg::rrf_fuse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(vg::kRrfMax * sizeof(uint64_t))));
        VG_LAUNCH(vg::rrf_fuse_kernel, dim3(static_cast<unsigned>(nq)), dim3(vg::kRrfThreads), lds, st, has_a ? da.ptr : nullptr,
                  has_a ? dca.ptr : nullptr, a_stride, has_b ? db.ptr : nullptr, has_b ? dcb.ptr : nullptr, b_stride, rrf_k, k, oid.ptr, osc.ptr,
                  ocnt.ptr);
    }
    VG_TRY(oid.finish());
    VG_TRY(osc.finish());
    VG_TRY(ocnt.finish());
    if (da.owned || db.owned || dca.owned || dcb.owned) VG_HIP(hipStreamSynchronize(st));  // the caller's host arrays have been read
    return VG_OK;
}
