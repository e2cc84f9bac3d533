// k_vamana_build.hip — Vamana construction on the GPU: diskann.Writer.buildGraph (internal/segment/diskann/
// writer.go:362-460) with its greedySearch (:472-569), robustPrune (:571-625) and addBackEdge (:627-643).
//
// The semantics are the header's (vg_vamana_build): centroid and entry point as the writer computes them, an
// initial graph from the shared counter RNG in place of rand.Perm, two passes (alpha 1, then alpha), nodes in
// id order in batches of clamp(processed / growth_div, 1, max_batch).  Every node of a batch searches the graph
// as it stood when the batch began and prunes its own list as it stood then; the new lists are written, then the
// back edges are applied per target in (source id, slot) order.  max_batch = 1 is the writer's sequential loop.
// Every sort is by the canonical (distance, id) key: -0 equals +0, every NaN after +Inf, ties by id.
// Per batch:
//   1. vb_search_kernel     one wavefront per node: greedySearch with the pool kept sorted in LDS (a merge of the
//                           expanded node's fresh neighbours per round, which is what sorting every round yields);
//                           a visited bitmap of n bits per node in HBM.
//   2. vb_prune_kernel      one workgroup per node: robustPrune over the search's l results and the old list.
//   3. vb_write_kernel      the new lists into the graph; one back-edge record per (node, slot).
//   4. the records are grouped by target (vg_group_records.hpp); vb_link_kernel: one workgroup per target sorts its
//      records by record index (= (source, slot) order) and applies addBackEdge to its list in LDS.
// Every distance is the reference's pair kernel in its summation order (vg_exact.hpp, distance.Provider).
#include <algorithm>
#include <cfloat>
#include <vector>

#include "vg_build_plan.hpp"
#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_group_records.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"
#include "vg_vamana_common.hpp"

namespace vg {

constexpr uint32_t kVbExpanded = 0x80000000u;  // pool entries: bit 31 of the id (ids < 2^31) = expanded
// purpose constant of the initial graph's draws: rng_u64(seed, node, kVamanaInitPurpose, t) (header)
constexpr uint64_t kVamanaInitPurpose = 0x56414D414E41ull;  // "VAMANA"

// ---- centroid, entry point, initial graph ------------------------------------------------------------
__global__ void vb_centroid_kernel(const float *__restrict__ base, int64_t n, int dim, float *__restrict__ c)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= dim) return;
    float s = 0.0f;
    for (int64_t i = 0; i < n; i++) s += base[i * dim + j];  // row order (writer.go:388-392)
    c[j] = s / static_cast<float>(n);
}

// the first row with dist(row, centroid) < minDist (minDist from MaxFloat32) = the least (canonical key) among the
// rows whose distance is below MaxFloat32; *best stays kKeyMax (entry 0) when there is none
__global__ __launch_bounds__(kVamanaThreads) void vb_entry_kernel(const float *__restrict__ base, int64_t n, int dim, bool dot,
                                                                  const float *__restrict__ c, unsigned long long *__restrict__ best)
{
    const int tid = threadIdx.x;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * (kVamanaThreads / 16) + (tid >> 4);
    if (row >= n) return;  // whole 16-lane groups leave together
    const float d = vb_pair(base + row * dim, c, dim, dot, Sub16::make(tid));
    if ((tid & 15) == 0 && d < FLT_MAX) atomicMin(best, static_cast<unsigned long long>(vb_key(d, static_cast<uint32_t>(row))));
}

__global__ void vb_init_kernel(int64_t n, int r, uint64_t seed, uint32_t *__restrict__ graph)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t *row = graph + i * r;
    const int want = static_cast<int>(std::min<int64_t>(r, n - 1));
    int cnt = 0;
    for (uint64_t t = 0; cnt < want; t++) {
        const uint32_t j = static_cast<uint32_t>(vb_rng_u64(seed, static_cast<uint64_t>(i), kVamanaInitPurpose, t) % static_cast<uint64_t>(n));
        if (j == static_cast<uint32_t>(i)) continue;
        bool dup = false;
        for (int s = 0; s < cnt; s++) dup |= row[s] == j;
        if (!dup) row[cnt++] = j;
    }
    for (int s = cnt; s < r; s++) row[s] = VG_INVALID_ID;
}

// ---- 1. greedySearch ---------------------------------------------------------------------------------
// the number of entries of a[0..len) whose key (flag masked) is below v
__device__ __forceinline__ int vb_count_below(const uint64_t *a, int len, uint64_t v)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((a[mid] & ~static_cast<uint64_t>(kVbExpanded)) < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One wavefront per node t0 + blockIdx.x.  LDS: two pools of l + 50 + r keys (ping-pong) and 64 fresh keys.
__global__ __launch_bounds__(64) void vb_search_kernel(const float *__restrict__ base, int64_t n, int dim, bool dot,
                                                        const uint32_t *__restrict__ graph, int r, int l, uint32_t entry,
                                                        int64_t node0, uint32_t *__restrict__ vis, int64_t vis_words,
                                                        uint32_t *__restrict__ res)
{
    extern __shared__ uint64_t vb_lds[];
    const int cap = l + 50 + r;
    uint64_t *pa = vb_lds, *pb = vb_lds + cap, *fresh = vb_lds + 2 * cap;
    const int lane = threadIdx.x;
    const Sub16 sub = Sub16::make(lane);
    const int grp = lane >> 4;
    const int64_t node = node0 + blockIdx.x;
    const float *q = base + node * dim;
    uint32_t *vw = vis + static_cast<int64_t>(blockIdx.x) * vis_words;
    {
        const float d = vb_pair(base + static_cast<int64_t>(entry) * dim, q, dim, dot, sub);
        if (lane == 0) {
            pa[0] = vb_key(d, entry);
            vw[entry >> 5] |= 1u << (entry & 31);
        }
    }
    int len = 1;
    __syncthreads();
    for (;;) {
        // the first unexpanded entry; none within the first l ends the search (writer.go:512-534)
        const int lim = min(len, l);
        int cur = -1;
        for (int b0 = 0; b0 < lim; b0 += 64) {
            const int i = b0 + lane;
            const bool un = i < lim && !(static_cast<uint32_t>(pa[i]) & kVbExpanded);
            const uint64_t m = __ballot(un);
            if (m) {
                cur = b0 + __builtin_ctzll(m);
                break;
            }
        }
        if (cur < 0) break;
        const uint32_t cnode = static_cast<uint32_t>(pa[cur]);
        __syncthreads();
        if (lane == 0) pa[cur] |= kVbExpanded;
        if (len > l + 50) len = l + 50;
        // its unvisited neighbours, in list order (lists hold unique ids, so the lanes do not collide)
        uint32_t nb = lane < r ? graph[static_cast<int64_t>(cnode) * r + lane] : VG_INVALID_ID;
        bool isnew = false;
        if (nb != VG_INVALID_ID) {
            const uint32_t bit = 1u << (nb & 31);
            isnew = !(atomicOr(&vw[nb >> 5], bit) & bit);
        }
        const uint64_t nm = __ballot(isnew);
        const int nf = __popcll(nm);
        if (isnew) fresh[__popcll(nm & ((1ull << lane) - 1))] = nb;
        __syncthreads();
        for (int f0 = 0; f0 < nf; f0 += 4) {
            const int f = f0 + grp;
            uint32_t id = 0;
            if (f < nf) id = static_cast<uint32_t>(fresh[f]);
            __syncthreads();
            if (f < nf) {
                const float d = vb_pair(base + static_cast<int64_t>(id) * dim, q, dim, dot, sub);
                if ((lane & 15) == 0) fresh[f] = vb_key(d, id);
            }
            __syncthreads();
        }
        if (nf == 0) continue;
        if (lane >= nf) fresh[lane] = kKeyMax;
        __syncthreads();
        bitonic_sort_lds(fresh, 64, lane, 64);
        // merge pool[0..len) and fresh[0..nf) into pb (keys unique: every id is in the pool at most once)
        for (int i = lane; i < len; i += 64) {
            const uint64_t v = pa[i];
            pb[i + vb_count_below(fresh, nf, v & ~static_cast<uint64_t>(kVbExpanded))] = v;
        }
        if (lane < nf) pb[lane + vb_count_below(pa, len, fresh[lane])] = fresh[lane];
        len += nf;
        __syncthreads();
        uint64_t *t = pa;
        pa = pb;
        pb = t;
    }
    // the first l ids of the sorted pool
    uint32_t *out = res + static_cast<int64_t>(blockIdx.x) * l;
    for (int i = lane; i < l; i += 64) out[i] = i < len ? (static_cast<uint32_t>(pa[i]) & ~kVbExpanded) : VG_INVALID_ID;
}

// ---- 2. robustPrune ----------------------------------------------------------------------------------
// vamana_select's rule for the writer's greedy selection (writer.go:598-617) over keys[0..np2) sorted, kKeyMax last: equal
// keys (one id seen twice) count once; candidate c is kept unless alpha * d(c, s) < d(c, node) for a kept s (fp32; NaN keeps it)
struct WriterRule {
    __device__ bool skip(const uint64_t *keys, int i, uint32_t) const { return i > 0 && keys[i - 1] == keys[i]; }
    __device__ bool occludes(float alpha, float dcs, float dist) const { return alpha * dcs < dist; }
};

// keys of candidates cands[0..nc) against node (invalid ids and the node itself drop out), padded to np2, sorted
__device__ void vb_keys(const float *__restrict__ base, int dim, bool dot, uint32_t node, const uint32_t *cands, int nc,
                        int np2, uint64_t *keys)
{
    const int tid = threadIdx.x, grp = tid >> 4;
    const Sub16 sub = Sub16::make(tid);
    const float *nv = base + static_cast<int64_t>(node) * dim;
    for (int c0 = 0; c0 < np2; c0 += kVamanaThreads / 16) {
        const int c = c0 + grp;
        uint64_t key = kKeyMax;
        if (c < nc) {
            const uint32_t id = cands[c];
            if (id != VG_INVALID_ID && id != node)
                key = vb_key(vb_pair(base + static_cast<int64_t>(id) * dim, nv, dim, dot, sub), id);
        }
        if ((tid & 15) == 0 && c < np2) keys[c] = key;
    }
    __syncthreads();
    bitonic_sort_lds(keys, np2, tid, kVamanaThreads);
}

// graph[i] = robustPrune(i, results ∪ graph[i], r, alpha) for node0 + blockIdx.x; LDS keys: np2 >= l + r
__global__ __launch_bounds__(kVamanaThreads) void vb_prune_kernel(const float *__restrict__ base, int dim, bool dot,
                                                                  const uint32_t *__restrict__ graph, int r, int l, float alpha,
                                                                  int64_t node0, const uint32_t *__restrict__ res, int np2,
                                                                  uint32_t *__restrict__ out)
{
    extern __shared__ uint64_t vb_lds[];
    __shared__ uint32_t cands[kVamanaMaxL + kVamanaMaxR];
    __shared__ uint32_t kept[kVamanaMaxR];
    __shared__ int flag, nkept;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const uint32_t node = static_cast<uint32_t>(node0 + b);
    for (int i = tid; i < l; i += kVamanaThreads) cands[i] = res[b * l + i];
    for (int i = tid; i < r; i += kVamanaThreads) cands[l + i] = graph[static_cast<int64_t>(node) * r + i];
    __syncthreads();
    vb_keys(base, dim, dot, node, cands, l + r, np2, vb_lds);
    const int nk = vamana_select(WriterRule{}, base, dim, dot, vb_lds, np2, r, alpha, kept, &flag, &nkept);
    for (int i = tid; i < r; i += kVamanaThreads) out[b * r + i] = i < nk ? kept[i] : VG_INVALID_ID;
}

// ---- 3. new lists, back-edge records -------------------------------------------------------------------
__global__ void vb_write_kernel(const uint32_t *__restrict__ lists, int64_t count, int r, int64_t node0,
                                uint32_t *__restrict__ graph)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < count * r) graph[node0 * r + i] = lists[i];
}

// ---- 4. back edges -----------------------------------------------------------------------------------
// One workgroup per target (vamana_link_target): addBackEdge(target, source) for each of its records: nothing if the source
// is listed, else append, and robustPrune(target, list, r, alpha) once the list is longer than r.
// LDS: the records (np2 of them, dynamic), the list.
__global__ __launch_bounds__(kVamanaThreads) void vb_link_kernel(const float *__restrict__ base, int dim, bool dot, int r,
                                                                 float alpha, int64_t node0, uint32_t *__restrict__ graph,
                                                                 const uint32_t *__restrict__ work,
                                                                 const GroupCounters *__restrict__ ctr, int32_t *__restrict__ rcnt,
                                                                 int32_t *__restrict__ rfill, const uint32_t *__restrict__ roff,
                                                                 const uint32_t *__restrict__ srt)
{
    extern __shared__ uint64_t vb_lds[];
    __shared__ uint64_t keys[2 * kVamanaMaxR];
    __shared__ uint32_t list[kVamanaMaxR + 1];
    __shared__ uint32_t kept[kVamanaMaxR];
    __shared__ int flag, nkept, cnt;
    // a list of r + 1: robustPrune(target, list, r, alpha)
    auto full = [&](uint32_t t, int nc) {
        vb_keys(base, dim, dot, t, list, nc, 2 * kVamanaMaxR, keys);
        const int nk = vamana_select(WriterRule{}, base, dim, dot, keys, 2 * kVamanaMaxR, r, alpha, kept, &flag, &nkept);
        for (int i = threadIdx.x; i < nk; i += kVamanaThreads) list[i] = kept[i];
        return nk;
    };
    vamana_link_target(r, node0, graph, work, ctr, rcnt, rfill, roff, srt, reinterpret_cast<uint32_t *>(vb_lds), list, &cnt, full);
}

// r, l, alpha of 0 become the defaults (vamana_check_rl); then every refusal vg_vamana_build makes before it allocates
// (vg_search.hpp: vg_diskann_build makes them before it quantizes)
int32_t vamana_build_check(const vg_index *idx, int32_t &r, int32_t &l, float &alpha, int32_t max_batch, int32_t growth_div)
{
    VG_TRY(vamana_check_rl("vg_vamana_build", "r", r, l, alpha));
    VG_CHECK(max_batch >= 1 && growth_div >= 1, VG_ERR_INVALID_ARG, "vg_vamana_build: max_batch and growth_div must be >= 1");
    VG_TRY(vamana_check_batch("vg_vamana_build", max_batch));
    VG_CHECK(idx->n > 0, VG_ERR_INVALID_ARG, "vg_vamana_build: no vectors to write (n = 0)");
    VG_CHECK(idx->n < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "vg_vamana_build: n=%lld must be below 2^31",
             static_cast<long long>(idx->n));
    VG_CHECK(idx->d_vectors, VG_ERR_NOT_READY, "vg_vamana_build: index has no fp32 vectors");
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    return VG_OK;
}

}  // namespace vg

VG_API int32_t vg_vamana_build(vg_index *idx, int32_t r, int32_t l, float alpha, const uint32_t *init_graph,
                               uint64_t seed, int32_t max_batch, int32_t growth_div, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_vamana_build: NULL index");
    VG_TRY(vg::vamana_build_check(idx, r, l, alpha, max_batch, growth_div));
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int64_t n = idx->n;
    const int dim = idx->dim;
    const bool dot = idx->metric != VG_METRIC_L2;  // Cosine and Dot: raw Dot, ascending (distance.go:97-106)
    const float *base = idx->d_vectors;

    vg::DevBuf<uint32_t> g;
    VG_TRY(g.alloc(static_cast<size_t>(n) * r));
    if (init_graph) {  // validated and compacted (empty slots dropped, order kept) on the host
        std::vector<uint32_t> h(static_cast<size_t>(n) * r);
        VG_HIP(hipMemcpyAsync(h.data(), init_graph, h.size() * 4, hipMemcpyDefault, st));
        VG_HIP(hipStreamSynchronize(st));
        std::vector<uint32_t> row;
        for (int64_t i = 0; i < n; i++) {
            row.clear();
            for (int s = 0; s < r; s++) {
                const uint32_t v = h[static_cast<size_t>(i) * r + s];
                if (v == VG_INVALID_ID) continue;
                VG_CHECK(v < n, VG_ERR_INVALID_ARG, "vg_vamana_build: init_graph[%lld][%d] = %u is not a row",
                         static_cast<long long>(i), s, v);
                VG_CHECK(v != static_cast<uint32_t>(i), VG_ERR_INVALID_ARG, "vg_vamana_build: init_graph row %lld links itself",
                         static_cast<long long>(i));
                VG_CHECK(std::find(row.begin(), row.end(), v) == row.end(), VG_ERR_INVALID_ARG,
                         "vg_vamana_build: init_graph row %lld lists %u twice", static_cast<long long>(i), v);
                row.push_back(v);
            }
            row.resize(static_cast<size_t>(r), VG_INVALID_ID);
            std::copy(row.begin(), row.end(), h.begin() + static_cast<size_t>(i) * r);
        }
        VG_HIP(hipMemcpyAsync(g.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
        VG_HIP(hipStreamSynchronize(st));
    } else {
        VG_LAUNCH(vg::vb_init_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, n, r, seed, g.p);
    }

    // centroid and entry point (writer.go:386-404)
    vg::DevBuf<float> cen;
    vg::DevBuf<unsigned long long> best;
    VG_TRY(cen.alloc(static_cast<size_t>(dim)));
    VG_TRY(best.alloc(1));
    VG_HIP(hipMemsetAsync(best.p, 0xFF, 8, st));
    VG_LAUNCH(vg::vb_centroid_kernel, dim3(static_cast<unsigned>((dim + 63) / 64)), dim3(64), 0, st, base, n, dim, cen.p);
    VG_LAUNCH(vg::vb_entry_kernel, dim3(static_cast<unsigned>((n + 15) / 16)), dim3(vg::kVamanaThreads), 0, st, base, n, dim,
              dot, cen.p, best.p);
    unsigned long long hbest = 0;
    VG_HIP(hipMemcpyAsync(&hbest, best.p, 8, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    const uint32_t entry = hbest == vg::kKeyMax ? 0u : static_cast<uint32_t>(hbest);

    // scratch: per batch node l results and r new slots (records), visited bitmaps; the call's own, freed at return
    vg::VamanaBatch bt(idx->ctx, n, std::min<int64_t>(max_batch, n), static_cast<size_t>(l) * 4, r);
    vg::DevBuf<char> scratch;
    VG_TRY(scratch.alloc(bt.carve(nullptr)));
    bt.carve(scratch.p);
    VG_TRY(bt.start_records(vg::vb_link_kernel, st));
    uint32_t *res = reinterpret_cast<uint32_t *>(bt.res);

    const size_t search_lds = static_cast<size_t>(2 * (l + 50 + r) + 64) * 8;
    const int prune_np2 = vg::next_pow2(l + r);
    const size_t prune_lds = static_cast<size_t>(prune_np2) * 8;
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vg::vb_search_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(search_lds)));
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vg::vb_prune_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(prune_lds)));

    int64_t processed = 0;
    for (int pass = 0; pass < 2; pass++) {  // writer.go:430-457
        const float a = pass == 0 ? 1.0f : alpha;
        for (int64_t t0 = 0; t0 < n;) {
            const int64_t b = vg::next_batch(processed, (pass + 1) * n, max_batch, growth_div);  // (= n - t0 at the most)
            {
                vg::ProfScope prof(idx->ctx, "vamana_build_search", st);
                VG_TRY(vg::for_each_walk_chunk(bt.vis, bt.vis_words, bt.chunk, b, st, [&](int64_t c0, int64_t cn) -> int32_t {
                    VG_LAUNCH(vg::vb_search_kernel, dim3(static_cast<unsigned>(cn)), dim3(64), search_lds, st, base, n, dim,
                              dot, g.p, r, l, entry, t0 + c0, bt.vis, bt.vis_words, res + c0 * l);
                    return VG_OK;
                }));
            }
            {
                vg::ProfScope prof(idx->ctx, "vamana_build_prune", st);
                VG_LAUNCH(vg::vb_prune_kernel, dim3(static_cast<unsigned>(b)), dim3(vg::kVamanaThreads), prune_lds, st, base,
                          dim, dot, g.p, r, l, a, t0, res, prune_np2, bt.nl);
                VG_LAUNCH(vg::vb_write_kernel, dim3(static_cast<unsigned>((b * r + 255) / 256)), dim3(256), 0, st, bt.nl,
                          b, r, t0, g.p);
            }
            {
                vg::ProfScope prof(idx->ctx, "vamana_build_backedge", st);
                VG_TRY(bt.reverse_edges(b, st, vg::vb_link_kernel, base, dim, dot, r, a, t0, g.p));
            }
            t0 += b;
            processed += b;
        }
    }
    VG_HIP(hipStreamSynchronize(st));
    if (idx->d_vamana) (void)hipFree(idx->d_vamana);
    idx->d_vamana = g.release();
    idx->vamana_cap = 0;
    idx->vamana_r = r;
    idx->vamana_entry = entry;
    return VG_OK;
}

VG_API int32_t vg_index_get_vamana_graph(const vg_index *idx, int32_t *r, uint32_t *entry_point, uint32_t *graph,
                                         void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_get_vamana_graph: NULL index");
    VG_CHECK(idx->d_vamana || idx->n == 0, VG_ERR_NOT_READY, "vg_index_get_vamana_graph: index has no Vamana graph");
    if (r) *r = idx->vamana_r;
    if (entry_point) *entry_point = idx->vamana_entry;
    if (graph && idx->n > 0 && idx->d_vamana) {
        VG_HIP(hipSetDevice(idx->ctx->device));
        hipStream_t st = vg::pick_stream(idx->ctx, stream);
        VG_HIP(hipMemcpyAsync(graph, idx->d_vamana, static_cast<size_t>(idx->n) * idx->vamana_r * 4, hipMemcpyDefault, st));
        VG_HIP(hipStreamSynchronize(st));
    }
    return VG_OK;
}
