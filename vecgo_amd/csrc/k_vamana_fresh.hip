// k_vamana_fresh.hip — the streaming Vamana index on the GPU: FreshVamana.Insert (internal/segment/diskann/
// fresh_vamana.go:178-222) with searchCandidatesLocked (:616-671), robustPruneLocked (:748-792), addReverseEdgeLocked
// (:698-745) and maybeUpdateEntryPoint (:795-801); FreshVamana.Search / SearchWithFilter (:272-364) with greedySearch
// (:535-613).  The semantics are the header's (vg_vamana_insert, vg_search_vamana_fresh).
//
// Both searches are one walk: two bounded lists sorted by (distance, arrival) — `candidates` (cap 2 ef, popped from the
// front) and `results` (cap ef) — and a stop once the popped distance exceeds the last of a full `results`.  The insert's
// results leave deleted nodes out, the query search's take every node: the walk kernel's compile-time flag.
// insertCandidate (:898-923) places an item after every entry whose distance is <= its own and drops it at position >= cap.
// Inserting a popped node's fresh neighbours one by one, cutting each time, leaves the list that ONE stable merge and one
// cut leave (an item cut early already has cap items at or before it, and later inserts only add more).  So a wavefront
// scores the <= 64 fresh neighbours in parallel, ranks them among themselves by (distance, list slot), and merges once per
// pop: a list entry moves up by the fresh entries BELOW it, a fresh entry by the list entries AT OR BELOW it; keys are
// compared on the distance word only.
// Per batch of the insert:
//   1. fv_walk_kernel<true>   one wavefront per node: the search, lists in LDS, a visited bitmap of n bits per node in HBM.
//   2. fv_prune_kernel        one workgroup per node: robustPrune over the results; writes the node's list and one
//                             reverse-edge record per slot.
//   3. the records are grouped by target (vg_group_records.hpp); fv_link_kernel: one workgroup per target sorts its records
//      by record index (= (source, slot) order) and applies addReverseEdge to its list in LDS.
// FreshVamana.consolidate (:803-867, vg_vamana_consolidate) is steps 1 and 2 for nodes already in the graph, no reverse edges:
//   fv_mark_kernel            one pass over the n x r table: a need-bit per live node that lists a deleted id, the counters.
//   per batch of the marked nodes (the host's ascending id list): fv_walk_kernel<true> and fv_prune_kernel over that list.
// Every distance is the reference's pair kernel in its summation order (vg_exact.hpp, distance.Provider).
#include <algorithm>
#include <cmath>
#include <vector>

#include "vg_build_plan.hpp"
#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_group_records.hpp"
#include "vg_grow_rows.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"
#include "vg_vamana_common.hpp"

namespace vg {

constexpr int kFvMaxEf = 2048;  // 6 ef keys of 8 bytes (two lists of 2 ef and ef, ping-ponged): 96 KiB of LDS

// bit i of byte i/8 = node i is deleted; the bitmap covers nodes below n_del, later nodes are live
__device__ __forceinline__ bool fv_deleted(const uint8_t *__restrict__ del, int64_t n_del, uint32_t id)
{
    return del && id < n_del && ((del[id >> 3] >> (id & 7)) & 1);
}

__device__ __forceinline__ uint32_t fv_word(uint64_t key) { return static_cast<uint32_t>(key >> 32); }

// how many of a[0..len) have a distance word below w (LE: at or below)
template <bool LE>
__device__ __forceinline__ int fv_count(const uint64_t *a, int len, uint32_t w)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t m = fv_word(a[mid]);
        if (LE ? m <= w : m < w) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// dst = the stable merge of src[0..len) and fs[0..nf) (an src entry before an fs entry of equal distance), cut at cap;
// the new length.  One wavefront; the caller puts a barrier after it.
__device__ __forceinline__ int fv_merge(const uint64_t *src, int len, const uint64_t *fs, int nf, uint64_t *dst, int cap, int lane)
{
    for (int i = lane; i < len; i += 64) {
        const uint64_t v = src[i];
        const int pos = i + fv_count<false>(fs, nf, fv_word(v));
        if (pos < cap) dst[pos] = v;
    }
    if (lane < nf) {
        const uint64_t v = fs[lane];
        const int pos = lane + fv_count<true>(src, len, fv_word(v));
        if (pos < cap) dst[pos] = v;
    }
    return min(len + nf, cap);
}

// ---- 1. searchCandidatesLocked / greedySearch ----------------------------------------------------------
// One wavefront per searching node or query blockIdx.x, whose vector is queries + blockIdx.x * dim, or with qids (the
// consolidate's repair list) row qids[blockIdx.x] of base.  INSERT: `results`
// leaves deleted nodes out and goes to res (ef keys, kKeyMax after the last).  Otherwise `results` takes every node and
// its first k entries that are neither deleted nor masked out go to ids / scores / counts.
// LDS (dynamic): candidates 2 x 2 ef keys, results 2 x ef keys, the fresh keys ranked for either list 2 x 64.
template <bool INSERT>
__global__ __launch_bounds__(64) void fv_walk_kernel(const float *__restrict__ base, int dim, bool dot,
                                                      const uint32_t *__restrict__ graph, int r, int ef, uint32_t entry,
                                                      const float *__restrict__ queries, const uint32_t *__restrict__ qids,
                                                      const uint8_t *__restrict__ deleted, int64_t n_del,
                                                      uint32_t *__restrict__ vis, int64_t vis_words,
                                                      uint64_t *__restrict__ res, int k, const uint8_t *__restrict__ mask,
                                                      int64_t mask_stride, float pad_score, uint32_t *__restrict__ ids,
                                                      float *__restrict__ scores, int32_t *__restrict__ counts)
{
    extern __shared__ uint64_t fv_lds[];
    __shared__ uint32_t nbs[64];
    __shared__ uint64_t fu[64];  // the fresh keys in arrival order
    const int ccap = 2 * ef;
    uint64_t *ca = fv_lds, *cb = ca + ccap, *ra = cb + ccap, *rb = ra + ef, *fc = rb + ef, *fr = fc + 64;
    const int lane = threadIdx.x;
    const Sub16 sub = Sub16::make(lane);
    const int grp = lane >> 4;
    const int64_t b = blockIdx.x;
    const float *q = qids ? base + static_cast<int64_t>(qids[b]) * dim : queries + b * dim;
    uint32_t *vw = vis + b * vis_words;
    int chead = 0, clen = 1, rlen = 0;
    {
        const float d = vb_pair(base + static_cast<int64_t>(entry) * dim, q, dim, dot, sub);
        const bool live = !INSERT || !fv_deleted(deleted, n_del, entry);
        if (lane == 0) {
            ca[0] = vb_key(d, entry);
            if (live) ra[0] = ca[0];
            vw[entry >> 5] |= 1u << (entry & 31);
        }
        rlen = live ? 1 : 0;
    }
    __syncthreads();
    while (clen > 0) {
        const uint64_t closest = ca[chead];
        chead++;
        clen--;
        if (rlen >= ef && fv_word(closest) > fv_word(ra[rlen - 1])) break;
        const uint32_t cnode = key_row(closest);
        // its unvisited neighbours in list order: empty slots skipped, an id listed twice counts at its first slot
        const uint32_t nb = lane < r ? graph[static_cast<int64_t>(cnode) * r + lane] : VG_INVALID_ID;
        __syncthreads();
        nbs[lane] = nb;
        __syncthreads();
        bool isnew = nb != VG_INVALID_ID;
        for (int j = 0; j < r; j++) isnew &= !(j < lane && nbs[j] == nb);
        if (isnew) {
            const uint32_t bit = 1u << (nb & 31);
            isnew = !(atomicOr(&vw[nb >> 5], bit) & bit);
        }
        const uint64_t nm = __ballot(isnew);
        const int nf = __popcll(nm);
        if (nf == 0) continue;
        const int slot = __popcll(nm & ((1ull << lane) - 1));
        __syncthreads();
        if (isnew) nbs[slot] = nb;
        __syncthreads();
        for (int f0 = 0; f0 < nf; f0 += 4) {
            const int f = f0 + grp;
            if (f < nf) {
                const uint32_t id = nbs[f];
                const float d = vb_pair(base + static_cast<int64_t>(id) * dim, q, dim, dot, sub);
                if ((lane & 15) == 0) fu[f] = vb_key(d, id);
            }
        }
        __syncthreads();
        // ranks among the fresh entries by (distance, arrival); for the results among those it takes
        const uint64_t mine = lane < nf ? fu[lane] : kKeyMax;
        const bool take = lane < nf && (!INSERT || !fv_deleted(deleted, n_del, key_row(mine)));
        const uint64_t tm = __ballot(take);
        const int nfr = __popcll(tm);
        int rank_c = 0, rank_r = 0;
        for (int j = 0; j < nf; j++) {
            const uint32_t wj = fv_word(fu[j]);
            const bool before = wj < fv_word(mine) || (wj == fv_word(mine) && j < lane);
            rank_c += before;
            rank_r += before && ((tm >> j) & 1);
        }
        if (lane < nf) fc[rank_c] = mine;
        if (take) fr[rank_r] = mine;
        __syncthreads();
        clen = fv_merge(ca + chead, clen, fc, nf, cb, ccap, lane);
        rlen = fv_merge(ra, rlen, fr, nfr, rb, ef, lane);
        chead = 0;
        __syncthreads();
        uint64_t *t = ca;
        ca = cb;
        cb = t;
        t = ra;
        ra = rb;
        rb = t;
    }
    if (INSERT) {
        uint64_t *out = res + b * ef;
        for (int i = lane; i < ef; i += 64) out[i] = i < rlen ? ra[i] : kKeyMax;
        return;
    }
    // the first k results that are not deleted and pass the filter (fresh_vamana.go:296-311, :342-360)
    const uint8_t *mk = mask ? mask + b * mask_stride : nullptr;
    uint32_t *oi = ids + b * k;
    float *os = scores + b * k;
    int kept = 0;
    for (int i0 = 0; i0 < rlen && kept < k; i0 += 64) {
        const int i = i0 + lane;
        const uint64_t key = i < rlen ? ra[i] : kKeyMax;
        const uint32_t id = key_row(key);
        const bool keep = i < rlen && !fv_deleted(deleted, n_del, id) && (!mk || ((mk[id >> 3] >> (id & 7)) & 1));
        const uint64_t m = __ballot(keep);
        const int at = kept + __popcll(m & ((1ull << lane) - 1));
        if (keep && at < k) {
            oi[at] = id;
            os[at] = key_score(key, false);
        }
        kept = min(k, kept + __popcll(m));
    }
    for (int i = kept + lane; i < k; i += 64) {
        oi[i] = VG_INVALID_ID;
        os[i] = pad_score;
    }
    if (lane == 0 && counts) counts[b] = kept;
}

// ---- 2. robustPruneLocked ------------------------------------------------------------------------------
// vamana_select's rule for the greedy selection of fresh_vamana.go:762-789 over the candidates in (distance, position)
// order, kKeyMax after the last: self and deleted ids are skipped; c is kept unless d(c, s) < alpha * c.dist for a kept s
// (the product is fp32 and its own rounding step; a false comparison, a NaN's included, keeps c)
struct FreshRule {
    uint32_t self;
    const uint8_t *__restrict__ deleted;  // restrict as the kernels' parameter is: without it the selection compiles to other code
    int64_t n_del;
    __device__ bool skip(const uint64_t *, int, uint32_t id) const { return id == self || fv_deleted(deleted, n_del, id); }
    __device__ bool occludes(float alpha, float dcs, float dist) const { return dcs < alpha * dist; }
};

// list(node) = robustPrune(node, its search results, r, alpha) for node = node0 + blockIdx.x, or nodes[blockIdx.x] with a
// list of nodes, into the graph; with nl, one reverse-edge record per slot; with links, the kept ids are counted
__global__ __launch_bounds__(kVamanaThreads) void fv_prune_kernel(const float *__restrict__ base, int dim, bool dot, int r, int l,
                                                                  float alpha, int64_t node0, const uint32_t *__restrict__ nodes,
                                                                  const uint64_t *__restrict__ res, const uint8_t *__restrict__ deleted,
                                                                  int64_t n_del, uint32_t *__restrict__ graph, uint32_t *__restrict__ nl,
                                                                  unsigned long long *__restrict__ links)
{
    __shared__ uint64_t ck[kVamanaMaxL];
    __shared__ uint32_t kept[kVamanaMaxR];
    __shared__ int flag, nkept;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const uint32_t node = nodes ? nodes[b] : static_cast<uint32_t>(node0 + b);
    for (int i = tid; i < l; i += kVamanaThreads) ck[i] = res[b * l + i];
    __syncthreads();
    const int nk = vamana_select(FreshRule{node, deleted, n_del}, base, dim, dot, ck, l, r, alpha, kept, &flag, &nkept);
    for (int i = tid; i < r; i += kVamanaThreads) {
        const uint32_t v = i < nk ? kept[i] : VG_INVALID_ID;
        graph[static_cast<int64_t>(node) * r + i] = v;
        if (nl) nl[b * r + i] = v;
    }
    if (links && tid == 0) atomicAdd(links, static_cast<unsigned long long>(nk));
}

// ---- 3. addReverseEdgeLocked ---------------------------------------------------------------------------
// One workgroup per target (vamana_link_target) applies addReverseEdge for each of its records: nothing if the source is
// listed; appended while the list is shorter than r; at r the list in slot order followed by the source, sorted stably by
// distance to the target, goes through robustPrune(target, ..., r, alpha), which drops deleted ids and may keep fewer than r.
// LDS: the records (np2 of them, dynamic), the list.
__global__ __launch_bounds__(kVamanaThreads) void fv_link_kernel(const float *__restrict__ base, int dim, bool dot, int r, float alpha,
                                                                 int64_t node0, const uint8_t *__restrict__ deleted, int64_t n_del,
                                                                 uint32_t *__restrict__ graph, const uint32_t *__restrict__ work,
                                                                 const GroupCounters *__restrict__ ctr, int32_t *__restrict__ rcnt,
                                                                 int32_t *__restrict__ rfill, const uint32_t *__restrict__ roff,
                                                                 const uint32_t *__restrict__ srt)
{
    extern __shared__ uint64_t fv_lds[];
    __shared__ uint64_t keys[2 * kVamanaMaxR];
    __shared__ uint64_t ck[kVamanaMaxR + 1];
    __shared__ uint32_t list[kVamanaMaxR + 1];
    __shared__ uint32_t kept[kVamanaMaxR];
    __shared__ int flag, nkept, cnt;
    // a list of r + 1: the candidates keyed (distance, position), sorted, then keyed (distance, id) for the prune
    auto full = [&](uint32_t t, int nc) {
        const int tid = threadIdx.x, grp = tid >> 4;
        const Sub16 sub = Sub16::make(tid);
        const float *tv = base + static_cast<int64_t>(t) * dim;
        for (int c0 = 0; c0 < 2 * kVamanaMaxR; c0 += kVamanaThreads / 16) {
            const int i = c0 + grp;
            uint64_t key = kKeyMax;
            if (i < nc) key = vb_key(vb_pair(tv, base + static_cast<int64_t>(list[i]) * dim, dim, dot, sub), static_cast<uint32_t>(i));
            if ((tid & 15) == 0) keys[i] = key;
        }
        __syncthreads();
        bitonic_sort_lds(keys, 2 * kVamanaMaxR, tid, kVamanaThreads);
        if (tid < nc) ck[tid] = (keys[tid] & 0xFFFFFFFF00000000ull) | list[key_row(keys[tid])];
        __syncthreads();
        const int nk = vamana_select(FreshRule{t, deleted, n_del}, base, dim, dot, ck, nc, r, alpha, kept, &flag, &nkept);
        for (int i = tid; i < nk; i += kVamanaThreads) list[i] = kept[i];
        return nk;
    };
    vamana_link_target(r, node0, graph, work, ctr, rcnt, rfill, roff, srt, reinterpret_cast<uint32_t *>(fv_lds), list, &cnt, full);
}

// ---- 4. consolidate's repair set (fresh_vamana.go:836-847) ---------------------------------------------
// One pass over the n x r table.  A wavefront owns one word of need = 32 consecutive nodes = one contiguous run of 32 r
// slots, and reads it 64 lanes at a time: g lanes per node (g = r rounded up to a power of two, at least 2), each lane one
// slot, 64 / g whole nodes per step.  A live node with a deleted id in any non-empty slot gets its bit; the word is stored
// once, whole (no atomics, nothing to clear).  ctr[0..3) += such nodes, their slots that name a deleted id, their non-empty
// slots: summed per wavefront in registers, per workgroup in LDS, then one atomicAdd each per workgroup that found any.
__global__ __launch_bounds__(kVamanaThreads) void fv_mark_kernel(const uint32_t *__restrict__ graph, int64_t n, int r, int g,
                                                                 const uint8_t *__restrict__ deleted, uint32_t *__restrict__ need,
                                                                 unsigned long long *__restrict__ ctr)
{
    __shared__ unsigned int tot[3];
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t word = static_cast<int64_t>(blockIdx.x) * (kVamanaThreads / 64) + (threadIdx.x >> 6);
    if (word * 32 < n) {  // uniform over the wavefront
        const int per = 64 / g, slot = lane & (g - 1), sub = lane >> __builtin_ctz(g);
        const uint64_t mine = (g == 64 ? ~0ull : (1ull << g) - 1) << (lane & ~(g - 1));
        uint32_t bits = 0;
        unsigned int nodes = 0, dropped = 0, before = 0;
        for (int s = 0; s < 32; s += per) {
            const int64_t node = word * 32 + s + sub;
            uint32_t id = VG_INVALID_ID;
            if (node < n && slot < r && !fv_deleted(deleted, n, static_cast<uint32_t>(node))) id = graph[node * r + slot];
            const bool linked = id != VG_INVALID_ID;  // a non-empty slot of a live node
            const uint64_t dead = __ballot(linked && fv_deleted(deleted, n, id));
            const bool repair = (dead & mine) != 0;
            const uint64_t heads = __ballot(repair && slot == 0);  // bit j g = node s + j is to be repaired: folded to bit j
            const uint64_t fold = __ballot(lane < per && ((heads >> (lane < per ? lane * g : 0)) & 1));
            bits |= static_cast<uint32_t>(fold) << s;
            nodes += __popcll(heads);
            dropped += __popcll(dead);
            before += __popcll(__ballot(repair && linked));
        }
        if (lane == 0) {
            need[word] = bits;
            if (nodes) {
                atomicAdd(&tot[0], nodes);
                atomicAdd(&tot[1], dropped);
                atomicAdd(&tot[2], before);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 && tot[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], static_cast<unsigned long long>(tot[threadIdx.x]));
}

template <bool INSERT>
static int32_t fv_walk_lds(int ef, size_t *lds)
{
    *lds = static_cast<size_t>(6 * ef + 128) * 8;
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fv_walk_kernel<INSERT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(*lds)));
    return VG_OK;
}

// The searches of nodes c0 .. c0 + cn - 1 of a batch (VamanaBatch::search), whose vectors are the rows from `queries` on or
// the rows qids[0..) of base; l result keys each into bt.res.  (The query search's outputs are not the insert walk's.)
static int32_t fv_insert_walk(const VamanaBatch &bt, int64_t c0, int64_t cn, size_t walk_lds, hipStream_t st, const float *base, int dim,
                              bool dot, const uint32_t *g, int r, int l, uint32_t entry, const float *queries, const uint32_t *qids,
                              const uint8_t *deleted, int64_t n_del)
{
    VG_LAUNCH(fv_walk_kernel<true>, dim3(static_cast<unsigned>(cn)), dim3(64), walk_lds, st, base, dim, dot, g, r, l, entry,
              queries ? queries + c0 * dim : nullptr, qids ? qids + c0 : nullptr, deleted, n_del, bt.vis, bt.vis_words,
              reinterpret_cast<uint64_t *>(bt.res) + c0 * l, 0, nullptr, int64_t(0), 0.0f, nullptr, nullptr, nullptr);
    return VG_OK;
}

}  // namespace vg

VG_API int32_t vg_vamana_insert(vg_index *idx, const float *rows, int64_t count, int32_t r, int32_t l, float alpha,
                                const uint8_t *deleted, uint64_t seed, int32_t max_batch, int32_t growth_div, void *stream)
{
    const char *fn = "vg_vamana_insert";
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(count >= 0 && (count == 0 || rows), VG_ERR_INVALID_ARG, "%s: count=%lld is negative, or rows is NULL", fn,
             static_cast<long long>(count));
    const int64_t n_old = idx->n;
    VG_CHECK(n_old == 0 || (idx->d_vectors && idx->d_vamana), VG_ERR_NOT_READY,
             "%s: the index has %lld rows but no Vamana graph (vg_vamana_build or vg_index_set_vamana_graph first)", fn,
             static_cast<long long>(n_old));
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    VG_TRY(vg::vamana_check_rl(fn, "r", r, l, alpha));
    VG_TRY(vg::vamana_check_batch(fn, max_batch));
    VG_CHECK(n_old + count < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "%s: %lld rows after the insert, must be below 2^31", fn,
             static_cast<long long>(n_old + count));
    VG_CHECK(max_batch >= 1 && growth_div >= 1, VG_ERR_INVALID_ARG, "%s: max_batch=%d and growth_div=%d must be >= 1", fn,
             max_batch, growth_div);
    VG_CHECK(n_old == 0 || r == idx->vamana_r, VG_ERR_INVALID_ARG, "%s: r=%d does not match the graph's (r=%d)", fn, r,
             idx->vamana_r);
    const char *held = vg::held_fresh_state(idx);
    VG_CHECK(!held, VG_ERR_UNSUPPORTED, "%s: the index holds %s, which the new rows would lack (segment state, not a "
             "streaming index's)", fn, held);
    if (count == 0) return VG_OK;
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int64_t n_new = n_old + count;
    const int dim = idx->dim;
    const bool dot = idx->metric != VG_METRIC_L2;  // Cosine and Dot: raw Dot, ascending (distance.go:97-106)

    // the batches and the entry point each starts from: all of it follows from the ids and the seed (vg_build_plan.hpp)
    const vg::FreshInsertPlan plan = vg::plan_fresh_insert(n_old, count, max_batch, growth_div, seed, idx->vamana_entry);

    // ---- the rows and everything sized by n ----
    vg::DevIn<float> in;
    vg::DevIn<uint8_t> del;
    VG_TRY(in.init(rows, static_cast<size_t>(count) * dim, st));
    VG_TRY(del.init(deleted, deleted ? static_cast<size_t>((n_old + 7) / 8) : 0, st, vg::kAnyAlign));
    VG_TRY(vg::append_index_rows(idx, in.ptr, count, st));
    VG_TRY(vg::grow_rows(&idx->d_vamana, &idx->vamana_cap, n_old, n_new, [&](int64_t x) { return static_cast<size_t>(x) * r * 4; }, st));
    VG_HIP(hipMemsetAsync(idx->d_vamana + n_old * r, 0xFF, static_cast<size_t>(count) * r * 4, st));
    const float *base = idx->d_vectors;
    uint32_t *g = idx->d_vamana;

    // ---- per-call scratch on the context arena: per batch node l result keys and r records, visited bitmaps
    vg::VamanaBatch bs(idx->ctx, n_new, plan.max_b, static_cast<size_t>(l) * 8, r);
    vg::ArenaCall ar(idx->ctx, st);
    const int a_bs = ar.add(bs.carve(nullptr));
    VG_TRY(ar.commit());
    bs.carve(ar.get<char>(a_bs));
    VG_TRY(bs.start_records(vg::fv_link_kernel, st));
    size_t walk_lds = 0;
    VG_TRY(vg::fv_walk_lds<true>(l, &walk_lds));

    for (const vg::BuildBatch &bt : plan.batches) {
        const int64_t t0 = bt.t0, b = bt.size;
        {
            vg::ProfScope prof(idx->ctx, "vamana_insert_search", st);
            VG_TRY(vg::for_each_walk_chunk(bs.vis, bs.vis_words, bs.chunk, b, st, [&](int64_t c0, int64_t cn) {
                return vg::fv_insert_walk(bs, c0, cn, walk_lds, st, base, dim, dot, g, r, l, bt.entry, base + t0 * dim, nullptr, del.ptr,
                                          n_old);
            }));
        }
        {
            vg::ProfScope prof(idx->ctx, "vamana_insert_prune", st);
            VG_LAUNCH(vg::fv_prune_kernel, dim3(static_cast<unsigned>(b)), dim3(vg::kVamanaThreads), 0, st, base, dim, dot, r, l, alpha,
                      t0, nullptr, reinterpret_cast<const uint64_t *>(bs.res), del.ptr, n_old, g, bs.nl, nullptr);
        }
        {
            vg::ProfScope prof(idx->ctx, "vamana_insert_reverse", st);
            VG_TRY(bs.reverse_edges(b, st, vg::fv_link_kernel, base, dim, dot, r, alpha, t0, del.ptr, n_old, g));
        }
    }
    VG_HIP(hipStreamSynchronize(st));
    idx->vamana_r = r;
    idx->vamana_entry = plan.entry;
    idx->n = n_new;
    return VG_OK;
}

VG_API int32_t vg_vamana_consolidate(vg_index *idx, int32_t l, float alpha, const uint8_t *deleted, int32_t max_batch,
                                     vg_vamana_consolidate_stats *stats, void *stream)
{
    const char *fn = "vg_vamana_consolidate";
    const vg_vamana_consolidate_stats none{0, 0, 0, 0};
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    const int64_t n = idx->n;
    if (n == 0) {  // consolidate returns on an empty index (:815-818)
        if (stats) *stats = none;
        return VG_OK;
    }
    VG_CHECK(idx->d_vectors && idx->d_vamana, VG_ERR_NOT_READY, "%s: index has no fp32 vectors or no Vamana graph", fn);
    int32_t r = idx->vamana_r;
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    VG_TRY(vg::vamana_check_rl(fn, "the graph's r", r, l, alpha));
    VG_TRY(vg::vamana_check_batch(fn, max_batch));
    VG_CHECK(max_batch >= 1, VG_ERR_INVALID_ARG, "%s: max_batch=%d must be >= 1", fn, max_batch);
    if (!deleted) {  // nothing is deleted: nothing to repair
        if (stats) *stats = none;
        return VG_OK;
    }
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int dim = idx->dim;
    const bool dot = idx->metric != VG_METRIC_L2;  // Cosine and Dot: raw Dot, ascending (distance.go:97-106)
    const float *base = idx->d_vectors;
    uint32_t *g = idx->d_vamana;
    vg::DevIn<uint8_t> del;
    VG_TRY(del.init(deleted, static_cast<size_t>((n + 7) / 8), st, vg::kAnyAlign));

    // ---- per-call scratch on the context arena: the need bits, the repair list (at most n ids), per batch node l result
    // keys and the visited bitmaps (no records)
    vg::VamanaBatch bs(idx->ctx, n, std::min<int64_t>(max_batch, n), static_cast<size_t>(l) * 8, 0);
    const int64_t vis_words = bs.vis_words;
    vg::ArenaCall ar(idx->ctx, st);
    const int a_need = ar.add(static_cast<size_t>(vis_words) * 4), a_rep = ar.add(static_cast<size_t>(n) * 4),
              a_bs = ar.add(bs.carve(nullptr)), a_ctr = ar.add(4 * sizeof(unsigned long long));
    VG_TRY(ar.commit());
    bs.carve(ar.get<char>(a_bs));
    uint32_t *need = ar.get<uint32_t>(a_need), *d_rep = ar.get<uint32_t>(a_rep);
    unsigned long long *ctr = ar.get<unsigned long long>(a_ctr);

    // ---- which nodes: fixed before the first repair (a repair rewrites only the node's own list) ----
    VG_HIP(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), st));
    {
        vg::ProfScope prof(idx->ctx, "vamana_consolidate_mark", st);
        const int waves = vg::kVamanaThreads / 64;  // one word of need each
        VG_LAUNCH(vg::fv_mark_kernel, dim3(static_cast<unsigned>((vis_words + waves - 1) / waves)), dim3(vg::kVamanaThreads), 0, st, g,
                  n, r, std::max(2, vg::next_pow2(r)), del.ptr, need, ctr);
    }
    std::vector<uint32_t> h_need(static_cast<size_t>(vis_words)), rep;
    VG_HIP(hipMemcpyAsync(h_need.data(), need, h_need.size() * 4, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));  // the host plans the launches from the count
    for (int64_t w = 0; w < vis_words; w++)
        for (uint32_t m = h_need[static_cast<size_t>(w)]; m; m &= m - 1)
            rep.push_back(static_cast<uint32_t>(w * 32 + __builtin_ctz(m)));
    const int64_t nrep = static_cast<int64_t>(rep.size());
    if (nrep == 0) {
        if (stats) *stats = none;
        return VG_OK;
    }
    VG_HIP(hipMemcpyAsync(d_rep, rep.data(), rep.size() * 4, hipMemcpyHostToDevice, st));

    // ---- batches of max_batch marked nodes in id order, each over the graph as it stood when the batch began ----
    size_t walk_lds = 0;
    VG_TRY(vg::fv_walk_lds<true>(l, &walk_lds));
    for (int64_t b0 = 0; b0 < nrep; b0 += max_batch) {
        const int64_t b = std::min<int64_t>(max_batch, nrep - b0);
        {
            vg::ProfScope prof(idx->ctx, "vamana_consolidate_search", st);
            VG_TRY(vg::for_each_walk_chunk(bs.vis, bs.vis_words, bs.chunk, b, st, [&](int64_t c0, int64_t cn) {
                return vg::fv_insert_walk(bs, c0, cn, walk_lds, st, base, dim, dot, g, r, l, idx->vamana_entry, nullptr, d_rep + b0,
                                          del.ptr, n);
            }));
        }
        vg::ProfScope prof(idx->ctx, "vamana_consolidate_prune", st);
        VG_LAUNCH(vg::fv_prune_kernel, dim3(static_cast<unsigned>(b)), dim3(vg::kVamanaThreads), 0, st, base, dim, dot, r, l, alpha,
                  int64_t(0), d_rep + b0, reinterpret_cast<const uint64_t *>(bs.res), del.ptr, n, g, nullptr, ctr + 3);
    }
    unsigned long long h_ctr[4] = {0, 0, 0, 0};
    VG_HIP(hipMemcpyAsync(h_ctr, ctr, sizeof h_ctr, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    if (stats)
        *stats = vg_vamana_consolidate_stats{static_cast<int64_t>(h_ctr[0]), static_cast<int64_t>(h_ctr[1]),
                                             static_cast<int64_t>(h_ctr[2]), static_cast<int64_t>(h_ctr[3])};
    return VG_OK;
}

VG_API int32_t vg_search_vamana_fresh(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t l,
                                      const uint8_t *deleted, const uint8_t *mask, int64_t mask_stride, uint32_t *ids,
                                      float *scores, int32_t *counts, void *stream)
{
    const char *fn = "vg_search_vamana_fresh";
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(nq >= 0 && k >= 0, VG_ERR_INVALID_ARG, "%s: negative nq or k", fn);
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(idx->n == 0 || (idx->d_vamana && idx->d_vectors), VG_ERR_NOT_READY, "%s: index has no Vamana graph or no fp32 vectors", fn);
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    VG_CHECK(queries && ids && scores, VG_ERR_INVALID_ARG, "%s: NULL buffer", fn);
    if (l == 0) l = 100;
    VG_CHECK(l >= 1, VG_ERR_INVALID_ARG, "%s: l=%d must be positive", fn, l);
    // Search: ef = max(2k, l) (:284-287); SearchWithFilter: ef = max(10k, 2l) (:331-334)
    const int64_t ef64 = mask ? std::max<int64_t>(int64_t(10) * k, int64_t(2) * l) : std::max<int64_t>(int64_t(2) * k, l);
    VG_CHECK(ef64 <= vg::kFvMaxEf, VG_ERR_UNSUPPORTED, "%s: ef=%lld (k=%d, l=%d) exceeds %d", fn, static_cast<long long>(ef64), k, l,
             vg::kFvMaxEf);
    VG_CHECK_MASK_STRIDE(fn, mask, mask_stride, idx->n);
    const int ef = static_cast<int>(ef64);
    const float pad = idx->metric != VG_METRIC_L2 ? -INFINITY : INFINITY;
    vg::SearchIO io;
    VG_TRY(io.init(idx->ctx, stream, queries, static_cast<size_t>(nq) * idx->dim, ids, scores, static_cast<size_t>(nq) * k, mask,
                   vg::mask_span(mask, mask_stride, nq, idx->n)));
    hipStream_t st = io.st;
    vg::DevIn<uint8_t> del;
    vg::DevOut<int32_t> ocnt;
    VG_TRY(del.init(deleted, deleted ? static_cast<size_t>((idx->n + 7) / 8) : 0, st, vg::kAnyAlign));
    VG_TRY(ocnt.init(counts, counts ? static_cast<size_t>(nq) : 0, st));
    if (idx->n == 0) {  // Search on an empty graph returns nothing (:280-282)
        uint32_t pad_bits;
        memcpy(&pad_bits, &pad, 4);
        VG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(io.oid.ptr), static_cast<int>(VG_INVALID_ID), static_cast<size_t>(nq) * k, st));
        VG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(io.osc.ptr), static_cast<int>(pad_bits), static_cast<size_t>(nq) * k, st));
        if (ocnt.ptr) VG_HIP(hipMemsetAsync(ocnt.ptr, 0, static_cast<size_t>(nq) * 4, st));
        VG_TRY(io.finish());
        return ocnt.finish();
    }
    size_t walk_lds = 0;
    VG_TRY(vg::fv_walk_lds<false>(ef, &walk_lds));
    vg::WalkChunks wc(vg::scratch_cap(idx->ctx), 0, idx->n, nq);
    vg::ArenaCall ar(idx->ctx, st);
    wc.add(ar);
    VG_TRY(ar.commit());
    const bool dot = idx->metric != VG_METRIC_L2;
    VG_TRY(wc.for_each(st, [&](int64_t q0, int64_t cnt) -> int32_t {
        vg::ProfScope prof(idx->ctx, "vamana_fresh_search", st);
        VG_LAUNCH(vg::fv_walk_kernel<false>, dim3(static_cast<unsigned>(cnt)), dim3(64), walk_lds, st, idx->d_vectors, idx->dim, dot,
                  idx->d_vamana, idx->vamana_r, ef, idx->vamana_entry, io.q.ptr + q0 * idx->dim, nullptr, del.ptr, idx->n, wc.vis(),
                  wc.vis_words, nullptr, k, io.mk.ptr ? io.mk.ptr + q0 * mask_stride : nullptr, mask_stride, pad,
                  io.oid.ptr + q0 * k, io.osc.ptr + q0 * k, ocnt.ptr ? ocnt.ptr + q0 : nullptr);
        return VG_OK;
    }));
    VG_TRY(io.finish());
    return ocnt.finish();
}
