// vg_vamana_common.hpp — what the two Vamana builders share (k_vamana_build.hip: the DiskANN writer's buildGraph;
// k_vamana_fresh.hip: the FreshVamana insert, consolidate and search).  On the device: the distance of a pair of rows and
// its sort key, the greedy selection of robustPrune (vamana_select, the two references' skip and occlusion tests as its
// rule), the per-target frame of the link kernels (vamana_link_target, what a full list does as its functor) and the fill
// of the edge records.  On the host: the limits, defaults and refusals of r / l / max_batch, and VamanaBatch, the scratch
// of a batched call with its chunked search loop and its reverse-edge stage.
#pragma once

#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_group_records.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"

namespace vg {

constexpr int kVamanaMaxR = 64;
constexpr int kVamanaMaxL = 1024;
constexpr int kVamanaMaxBatch = 16384;  // records of one target per batch are sorted in LDS (4 B each)
constexpr int kVamanaThreads = 256;

// canonical (distance, id) key: -0 -> +0, every NaN -> the positive quiet NaN (above +Inf)
__device__ __forceinline__ uint64_t vb_key(float d, uint32_t id)
{
    uint32_t u = __float_as_uint(d);
    if (d != d) u = 0x7FC00000u;
    else if (d == 0.0f) u = 0u;
    return make_key(__uint_as_float(u), id, false);
}

// distance.Provider(metric)(a, b): SquaredL2 or Dot in the pair kernel's order, all 16 lanes of a group
__device__ __forceinline__ float vb_pair(const float *a, const float *b, int dim, bool dot, Sub16 sub)
{
    return dot ? exact_pair16<true, kPair>(a, b, dim, sub) : exact_pair16<false, kPair>(a, b, dim, sub);
}

// The greedy selection of robustPrune over keys[0..nc): candidates in ascending order, kKeyMax after the last.  A candidate
// c that rule.skip(keys, i, id) does not drop is kept unless rule.occludes(alpha, d(c, s), d(c)) holds for a kept s (fp32;
// a false comparison, a NaN's included, keeps c); stops at r kept.  The references write the two tests in two forms with
// two roundings: the rules sit beside the kernels that cite them.
// Returns the number kept (kept[0..nk)); every thread of the workgroup.
template <class Rule>
__device__ int vamana_select(const Rule rule, const float *__restrict__ base, int dim, bool dot, const uint64_t *keys, int nc,
                             int r, float alpha, uint32_t *kept, int *flag, int *nkept)
{
    const int tid = threadIdx.x, grp = tid >> 4;
    const Sub16 sub = Sub16::make(tid);
    if (tid == 0) *nkept = 0;
    __syncthreads();
    for (int i = 0; i < nc; i++) {
        const uint64_t key = keys[i];
        const int nk = *nkept;
        if (key == kKeyMax || nk >= r) break;  // uniform
        const uint32_t id = key_row(key);
        if (rule.skip(keys, i, id)) continue;
        const float dist = key_score(key, false);
        const float *cv = base + static_cast<int64_t>(id) * dim;
        if (tid == 0) *flag = 0;
        __syncthreads();
        for (int s0 = 0; s0 < nk; s0 += kVamanaThreads / 16) {
            const int s = s0 + grp;
            if (s < nk) {
                const float dcs = vb_pair(cv, base + static_cast<int64_t>(kept[s]) * dim, dim, dot, sub);
                if ((tid & 15) == 0 && rule.occludes(alpha, dcs, dist)) *flag = 1;
            }
        }
        __syncthreads();
        if (tid == 0 && !*flag) {
            kept[nk] = id;
            *nkept = nk + 1;
        }
        __syncthreads();
    }
    return *nkept;
}

// records: rec[i] = target of record i (VG_INVALID_ID = none); record i = (source node0 + i / r, slot i % r); grouped by
// target (vg_group_records.hpp), the record's index as its payload (group_fill_index_kernel).
// The frame of a link kernel, one workgroup per target: its list without empty slots (an uploaded graph may hold holes),
// its records sorted by index (= (source, slot) order; the fill wrote them in any order), then for each source: nothing if
// it is listed; else appended, and once the list holds r + 1 entries full(target, r + 1) rewrites list[0..) and returns
// its new length (every thread).  The list goes back to the graph, rcnt / rfill are left zero for the next batch.
// LDS: order (the records padded to a power of two), list (r + 1 ids), cnt.
template <class Full>
__device__ void vamana_link_target(int r, int64_t node0, uint32_t *__restrict__ graph, const uint32_t *__restrict__ work,
                                   const GroupCounters *__restrict__ ctr, int32_t *__restrict__ rcnt, int32_t *__restrict__ rfill,
                                   const uint32_t *__restrict__ roff, const uint32_t *__restrict__ srt, uint32_t *order,
                                   uint32_t *list, int *cnt, Full full)
{
    if (blockIdx.x >= ctr->nwork) return;
    const int tid = threadIdx.x;
    const uint32_t t = work[blockIdx.x];
    const int nrec = rcnt[t];
    const uint32_t *mine = srt + roff[t];
    int np2 = 1;
    while (np2 < nrec) np2 <<= 1;
    for (int i = tid; i < np2; i += kVamanaThreads) order[i] = i < nrec ? mine[i] : 0xFFFFFFFFu;
    if (tid == 0) {
        int c = 0;
        for (int s = 0; s < r; s++) {
            const uint32_t v = graph[static_cast<int64_t>(t) * r + s];
            if (v != VG_INVALID_ID) list[c++] = v;
        }
        *cnt = c;
    }
    __syncthreads();
    bitonic_sort_lds(order, np2, tid, kVamanaThreads);
    for (int k = 0; k < nrec; k++) {
        const uint32_t src = static_cast<uint32_t>(node0 + order[k] / static_cast<uint32_t>(r));
        const int c = *cnt;
        if (__syncthreads_or(tid < c && list[tid] == src)) continue;  // already listed
        if (tid == 0) list[c] = src;
        __syncthreads();
        const int nc = c < r ? c + 1 : full(t, c + 1);
        if (tid == 0) *cnt = nc;
        __syncthreads();
    }
    const int c = *cnt;
    for (int i = tid; i < r; i += kVamanaThreads) graph[static_cast<int64_t>(t) * r + i] = i < c ? list[i] : VG_INVALID_ID;
    if (tid == 0) {
        rcnt[t] = 0;
        rfill[t] = 0;
    }
}

// The fill of the Vamana builders, whose payload is the record's index (the build's back edges, the FreshVamana insert's
// reverse edges; grouped by vg_group_records.hpp): srt[roff[row] ..] = the indices of the row's records, in any order (the link kernels sort them)
static __global__ void group_fill_index_kernel(const uint32_t *__restrict__ rec, int64_t nrec, const uint32_t *__restrict__ roff,
                                               int32_t *__restrict__ rfill, uint32_t *__restrict__ srt)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= nrec) return;
    const uint32_t t = rec[i];
    if (t == VG_INVALID_ID) return;
    srt[roff[t] + static_cast<uint32_t>(atomicAdd(&rfill[t], 1))] = static_cast<uint32_t>(i);
}

inline int next_pow2(int x)
{
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// ---- the host side of a batched call ---------------------------------------------------------------------------------
// r, l, alpha of 0 become the references' defaults (NewWriter, writer.go:84-95; FreshDefaultR / L / Alpha,
// fresh_vamana.go:20-24); then the refusals of r and l.  fn: the entry point the messages name; rname: "r", or whose r it is
// (a resident graph's is never 0).  The refusal of max_batch is a function of its own: vg_vamana_build makes another between.
inline int32_t vamana_check_rl(const char *fn, const char *rname, int32_t &r, int32_t &l, float &alpha)
{
    if (r == 0) r = 64;
    if (l == 0) l = 100;
    if (alpha == 0.0f) alpha = 1.2f;
    VG_CHECK(r >= 1 && r <= kVamanaMaxR, VG_ERR_UNSUPPORTED, "%s: %s=%d must be in 1..%d", fn, rname, r, kVamanaMaxR);
    VG_CHECK(l >= 1 && l <= kVamanaMaxL, VG_ERR_UNSUPPORTED, "%s: l=%d must be in 1..%d", fn, l, kVamanaMaxL);
    return VG_OK;
}
inline int32_t vamana_check_batch(const char *fn, int32_t max_batch)
{
    VG_CHECK(max_batch <= kVamanaMaxBatch, VG_ERR_UNSUPPORTED, "%s: max_batch=%d must be <= %d", fn, max_batch, kVamanaMaxBatch);
    return VG_OK;
}

// The scratch of a batched Vamana call over a graph of n rows in batches of at most max_b nodes, and the reverse-edge
// stage every builder runs over it.  Visited bitmaps for `chunk` searching nodes, as many as fit under the scratch cap (under
// the test hook VG_VAMANA_SMALL_SCRATCH: 64 KiB), the rest of a batch in further launches (for_each_walk_chunk,
// vg_search.hpp: node i of a launch from c0 over bitmap i - c0, into result row i); max_b result rows of res_bytes each;
// with records (r > 0: one per (node, slot)) the pieces of their grouping.  carve() as Carve does it: with a null base it
// returns the bytes, so the owner may be a DevBuf (the build: freed at return) or a piece of the context arena.
struct VamanaBatch {
    int64_t n, max_b, vis_words, chunk;
    size_t res_bytes;
    int r;  // records per node; 0: the call makes none
    uint32_t *vis = nullptr, *nl = nullptr, *work = nullptr, *srt = nullptr, *roff = nullptr;
    char *res = nullptr;
    int32_t *rcnt = nullptr, *rfill = nullptr;  // zero between batches: start_records() once, the link kernels leave them so
    GroupCounters *ctr = nullptr;
    VamanaBatch(const vg_ctx *ctx, int64_t n_, int64_t max_b_, size_t res_bytes_, int r_)
        : n(n_), max_b(max_b_), vis_words((n_ + 31) / 32),
          chunk(walk_chunk(hook(kHookVamanaSmallScratch) ? int64_t(64) << 10 : scratch_cap(ctx), vis_words * 4, max_b_)),
          res_bytes(res_bytes_), r(r_)
    {
    }
    size_t carve(char *base)
    {
        Carve c{base};
        c.take(vis, chunk * vis_words);
        c.take(res, max_b * static_cast<int64_t>(res_bytes));
        if (r == 0) return c.off;
        c.take(nl, max_b * r);
        c.take(work, std::min(max_b * r, n));
        c.take(srt, max_b * r);
        c.take(roff, n);
        c.take(rcnt, n);
        c.take(rfill, n);
        c.take(ctr, 1);
        return c.off;
    }
    size_t link_lds() const { return static_cast<size_t>(next_pow2(static_cast<int>(max_b))) * 4; }
    // before the first batch of a call with records: rcnt / rfill zero, and room for the link kernel's dynamic LDS (the
    // records one target can get in a batch, padded to a power of two)
    template <class Kernel>
    int32_t start_records(Kernel link, hipStream_t st) const
    {
        VG_HIP(hipMemsetAsync(rcnt, 0, static_cast<size_t>(n) * 4, st));
        VG_HIP(hipMemsetAsync(rfill, 0, static_cast<size_t>(n) * 4, st));
        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(link), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(link_lds())));
        return VG_OK;
    }
    // the reverse-edge stage of a batch of b: its records nl[0 .. b r) grouped by target, then the builder's link kernel, one
    // workgroup per target at the most, over its own leading arguments and the grouping
    template <class Kernel, class... Args>
    int32_t reverse_edges(int64_t b, hipStream_t st, Kernel link, Args... args) const
    {
        const int64_t nrec = b * r;
        const int64_t max_work = std::min(nrec, n);
        VG_TRY(group_count_offsets(nl, nrec, max_work, rcnt, work, roff, ctr, st));
        VG_LAUNCH(group_fill_index_kernel, dim3(static_cast<unsigned>((nrec + 255) / 256)), dim3(256), 0, st, nl, nrec, roff, rfill,
                  srt);
        VG_LAUNCH(link, dim3(static_cast<unsigned>(max_work)), dim3(kVamanaThreads), link_lds(), st, args..., work, ctr, rcnt, rfill,
                  roff, srt);
        return VG_OK;
    }
};

}  // namespace vg
