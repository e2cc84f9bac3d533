// k_vamana_reorder.hip — diskann.Writer.reorderBFS (internal/segment/diskann/reorder.go:14-157) on a resident index:
// the BFS order of the Vamana graph, then every per-row array the index holds permuted into it.
//
// Exact-order BFS.  The writer's queue visits level L+1 in the order its nodes are first discovered: parents in queue
// order p (the parent's position within level L), each parent's list in slot order j.  A node unvisited when level L
// began is enqueued at its first (p, j), so level L+1 sorted by min(p * r + j) over the slots that name it IS the
// queue's order.  Nodes discovered at level L+1 are exactly those unvisited at its start: a node visited earlier is
// skipped, a node of level L+1 already queued is skipped too (its key stays at the earlier slot).  The key of a slot
// names one node, so the minima of two nodes never tie, and "slot s is its node's minimum" marks every node of level
// L+1 exactly once.  Placing the winning slots in slot order therefore needs no sort: a prefix count of the winners.
//   rb_small_kernel     one workgroup of 256 threads walks every level of at most kRbSlots slots (S * r) without
//                       returning to the host: the minimum per node in an LDS hash table, the level's node list in LDS.
//                       It also walks the tail (reorder.go:57-82), i in id order: all ids below i are visited when
//                       the walk reaches i, so an unvisited i none of whose neighbours is both above i and unvisited
//                       is a component of one node; a batch of 256 ids places its prefix of such nodes at once, and
//                       the first id that is not such a node starts a BFS.  A path or an empty-list graph never
//                       leaves the kernel; it returns only at the end or at a level of more than kRbSlots slots.
//   rb_discover / rb_mark / rb_scan / rb_place   one such large level on the whole chip (one wavefront per parent,
//                       lane = slot): a 64-bit atomic min of p * r + j per node (reaches 2^37 at n < 2^31, r <= 64),
//                       the winning slots as a ballot mask per parent, an exclusive scan of their counts, the scatter.
//                       The host reads the state back once per such level only.
// Permutation: rb_gather_kernel<W> (vg_permute.hpp) moves rows of any size with W-byte accesses (16 where the row allows it),
// rb_graph_kernel gathers graph rows and maps every id through inv_perm, rb_tiles_kernel moves the 16-byte pieces of
// the tiled SQ8 layout between tiles.  The PQ and RaBitQ tiles are rebuilt from their permuted row-major copies.
#include <algorithm>
#include <vector>

#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_permute.hpp"
#include "vg_search.hpp"

namespace vg {

constexpr uint32_t kRbUnvisited = 0xFFFFFFFFu;
constexpr int kRbSlots = 2048;        // the largest level (S * r slots) the one-workgroup kernel walks
constexpr int kRbPer = kRbSlots / kRbThreads;
constexpr int kRbTableBits = 12;      // LDS hash table of node -> first slot: 2x the slots
constexpr int kRbTable = 1 << kRbTableBits;

struct RbState {
    uint32_t lo, hi;  // the current level is order[lo, hi); hi = nodes placed
    uint32_t root;    // the tail walk's next id: every id below it is visited
};

// inv / order are written and read back by the same workgroup inside rb_small_kernel: agent-scope accesses, so that
// every read sees the L2 and never a line the CU's vector cache kept from before the write
__device__ __forceinline__ uint32_t rb_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rb_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t rb_hash(uint32_t v) { return (v * 2654435761u) >> (32 - kRbTableBits); }

__global__ __launch_bounds__(kRbThreads) void rb_small_kernel(const uint32_t *__restrict__ g, int r, uint32_t n, uint32_t entry,
                                                              uint32_t *order, uint32_t *inv, RbState *state)
{
    __shared__ uint32_t tkey[kRbTable], tslot[kRbTable];
    __shared__ uint32_t lvl[2][kRbSlots];
    __shared__ uint32_t wsum[kRbThreads / 64];
    __shared__ uint32_t first;
    const int t = threadIdx.x;
    for (int i = t; i < kRbTable; i += kRbThreads) tkey[i] = tslot[i] = kRbUnvisited;
    RbState s = *state;
    if (s.hi == 0) {  // the main BFS opens at the entry point (reorder.go:33-35)
        if (t == 0) {
            rb_store(order, entry);
            rb_store(inv + entry, 0);
        }
        lvl[0][0] = entry;
        s.lo = 0;
        s.hi = 1;
    } else if (static_cast<uint64_t>(s.hi - s.lo) * r <= kRbSlots) {
        for (uint32_t i = t; i < s.hi - s.lo; i += kRbThreads) lvl[0][i] = rb_load(order + s.lo + i);
    }
    int cur = 0;
    __syncthreads();
    for (;;) {
        if (s.lo == s.hi) {  // the level is empty: the tail walk (reorder.go:57-82)
            if (s.hi >= n) break;
            bool opened = false;
            while (!opened && s.root < n) {
                const uint32_t i = s.root + t;
                bool single = false, stop = i >= n;
                if (!stop && rb_load(inv + i) == kRbUnvisited) {
                    // the row in chunks of 16 slots: every load of a chunk in flight at once
                    const uint32_t *row = g + static_cast<size_t>(i) * r;
                    bool blocked = false;
                    for (int j0 = 0; j0 < r && !blocked; j0 += 16) {
                        uint32_t w[16];
#pragma unroll
                        for (int c = 0; c < 16; c++) w[c] = j0 + c < r ? row[j0 + c] : kRbUnvisited;
#pragma unroll
                        for (int c = 0; c < 16; c++) w[c] = w[c] < n && w[c] > i ? rb_load(inv + w[c]) : 0u;
#pragma unroll
                        for (int c = 0; c < 16; c++) blocked |= w[c] == kRbUnvisited;
                    }
                    single = !blocked;
                    stop = blocked;
                }
                if (t == 0) first = kRbThreads;
                __syncthreads();
                if (stop) atomicMin(&first, static_cast<uint32_t>(t));
                __syncthreads();
                const uint32_t f = first;
                uint32_t total;
                const bool take = single && static_cast<uint32_t>(t) < f;
                const uint32_t rank = rb_block_scan(take ? 1u : 0u, wsum, &total);
                if (take) {
                    rb_store(order + s.hi + rank, i);
                    rb_store(inv + i, s.hi + rank);
                }
                s.hi += total;
                if (f < kRbThreads && s.root + f < n) {  // a BFS from root + f
                    const uint32_t root = s.root + f;
                    if (t == 0) {
                        rb_store(order + s.hi, root);
                        rb_store(inv + root, s.hi);
                    }
                    lvl[cur][0] = root;
                    s.lo = s.hi;
                    s.hi += 1;
                    s.root = root + 1;
                    opened = true;
                } else {
                    s.root = f < kRbThreads ? n : s.root + kRbThreads;
                }
                s.lo = opened ? s.lo : s.hi;
                __syncthreads();
            }
            if (!opened) break;  // (every id placed)
        }
        const uint32_t S = s.hi - s.lo;
        if (static_cast<uint64_t>(S) * r > kRbSlots) break;  // a large level: the whole chip takes it
        // this thread's slots: a contiguous run, so that thread order is slot order
        const uint32_t slots = S * r;
        const uint32_t per = (slots + kRbThreads - 1) / kRbThreads;
        const uint32_t s0 = t * per;
        uint32_t v[kRbPer], h[kRbPer];
#pragma unroll
        for (int c = 0; c < kRbPer; c++) {
            v[c] = kRbUnvisited;
            const uint32_t sl = s0 + c;
            if (c < static_cast<int>(per) && sl < slots) {
                const uint32_t p = sl / r, j = sl - p * r;
                const uint32_t w = g[static_cast<size_t>(lvl[cur][p]) * r + j];
                if (w < n && rb_load(inv + w) == kRbUnvisited) v[c] = w;
            }
        }
#pragma unroll
        for (int c = 0; c < kRbPer; c++) {
            if (v[c] == kRbUnvisited) continue;
            uint32_t hh = rb_hash(v[c]);
            for (;;) {
                const uint32_t old = atomicCAS(&tkey[hh], kRbUnvisited, v[c]);
                if (old == kRbUnvisited || old == v[c]) break;
                hh = (hh + 1) & (kRbTable - 1);
            }
            atomicMin(&tslot[hh], s0 + c);
            h[c] = hh;
        }
        __syncthreads();
        uint32_t win = 0, cnt = 0;
#pragma unroll
        for (int c = 0; c < kRbPer; c++)
            if (v[c] != kRbUnvisited && tslot[h[c]] == s0 + c) {
                win |= 1u << c;
                cnt++;
            }
        uint32_t total;
        uint32_t rank = rb_block_scan(cnt, wsum, &total);  // (its barriers: every tslot read is done below)
#pragma unroll
        for (int c = 0; c < kRbPer; c++) {
            if (v[c] == kRbUnvisited) continue;
            tkey[h[c]] = tslot[h[c]] = kRbUnvisited;
            if (win >> c & 1u) {
                rb_store(order + s.hi + rank, v[c]);
                rb_store(inv + v[c], s.hi + rank);
                lvl[cur ^ 1][rank] = v[c];
                rank++;
            }
        }
        __syncthreads();
        s.lo = s.hi;
        s.hi += total;
        cur ^= 1;
    }
    if (t == 0) *state = s;
}

// ---- one large level on the whole chip: one wavefront per parent, lane j = slot j -----------------------------------
__global__ __launch_bounds__(256) void rb_discover_kernel(const uint32_t *__restrict__ g, int r, uint32_t n,
                                                          const uint32_t *__restrict__ order, uint32_t lo, uint32_t S,
                                                          const uint32_t *__restrict__ inv, unsigned long long *keys)
{
    const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int j = threadIdx.x & 63;
    if (p >= S || j >= r) return;
    const uint32_t w = g[static_cast<size_t>(order[lo + p]) * r + j];
    if (w < n && inv[w] == kRbUnvisited) atomicMin(keys + w, static_cast<unsigned long long>(p) * r + j);
}

__global__ __launch_bounds__(256) void rb_mark_kernel(const uint32_t *__restrict__ g, int r, uint32_t n,
                                                      const uint32_t *__restrict__ order, uint32_t lo, uint32_t S,
                                                      const uint32_t *__restrict__ inv, const unsigned long long *__restrict__ keys,
                                                      unsigned long long *__restrict__ masks, uint32_t *__restrict__ counts)
{
    const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int j = threadIdx.x & 63;
    if (p >= S) return;  // (whole wavefronts)
    bool win = false;
    if (j < r) {
        const uint32_t w = g[static_cast<size_t>(order[lo + p]) * r + j];
        win = w < n && inv[w] == kRbUnvisited && keys[w] == static_cast<unsigned long long>(p) * r + j;
    }
    const unsigned long long m = __ballot(win);
    if (j == 0) {
        masks[p] = m;
        counts[p] = static_cast<uint32_t>(__popcll(m));
    }
}

// exclusive scan of counts[0, S) in place, one workgroup: a contiguous run per thread; the state moves to the next level
__global__ __launch_bounds__(kRbThreads) void rb_scan_kernel(uint32_t *counts, uint32_t S, RbState *state)
{
    __shared__ uint32_t wsum[kRbThreads / 64];
    const uint32_t per = (S + kRbThreads - 1) / kRbThreads;
    const uint32_t a = threadIdx.x * per, b = std::min(S, a + per);
    uint32_t sum = 0;
    for (uint32_t i = a; i < b; i++) sum += counts[i];
    uint32_t total;
    uint32_t run = rb_block_scan(sum, wsum, &total);
    for (uint32_t i = a; i < b; i++) {
        const uint32_t c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (threadIdx.x == 0) {
        RbState s = *state;
        s.lo = s.hi;
        s.hi += total;
        *state = s;
    }
}

__global__ __launch_bounds__(256) void rb_place_kernel(const uint32_t *__restrict__ g, int r, uint32_t *order, uint32_t lo,
                                                       uint32_t S, uint32_t hi, uint32_t *inv,
                                                       const unsigned long long *__restrict__ masks, const uint32_t *__restrict__ base)
{
    const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int j = threadIdx.x & 63;
    if (p >= S) return;
    const unsigned long long m = masks[p];
    if (!(m >> j & 1ull)) return;
    const uint32_t w = g[static_cast<size_t>(order[lo + p]) * r + j];
    const uint32_t pos = hi + base[p] + static_cast<uint32_t>(__popcll(m & ((1ull << j) - 1ull)));
    order[pos] = w;
    inv[w] = pos;
}

// ---- the permutation ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rb_map(uint32_t w, uint32_t n, const uint32_t *inv) { return w < n ? inv[w] : w; }

// graph row q = old row perm[q], every id through inv_perm (VG_INVALID_ID stays where it is); 4 slots per thread
// when r % 4 == 0
template <bool VEC>
__global__ __launch_bounds__(256) void rb_graph_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int64_t n, int r,
                                                       const uint32_t *__restrict__ perm, const uint32_t *__restrict__ inv)
{
    const int64_t words = VEC ? r / 4 : r, total = n * words;
    const uint32_t nn = static_cast<uint32_t>(n);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t q = e / words, k = e - q * words;
        if (VEC) {
            uint4 x = reinterpret_cast<const uint4 *>(src)[static_cast<int64_t>(perm[q]) * words + k];
            x.x = rb_map(x.x, nn, inv);
            x.y = rb_map(x.y, nn, inv);
            x.z = rb_map(x.z, nn, inv);
            x.w = rb_map(x.w, nn, inv);
            reinterpret_cast<uint4 *>(dst)[e] = x;
        } else {
            dst[e] = rb_map(src[static_cast<int64_t>(perm[q]) * words + k], nn, inv);
        }
    }
}

// tiled [tile][group][lane] 16-byte pieces (k_sq8_scan.hip's layout): piece (row q, group) = old piece (perm[q], group);
// the padding past n stays zero
__global__ __launch_bounds__(256) void rb_tiles_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int64_t n, int groups,
                                                       int64_t n_tiles, const uint32_t *__restrict__ perm)
{
    const int64_t total = n_tiles * groups * 64;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int lane = static_cast<int>(e & 63);
        const int64_t tg = e >> 6;
        const int gi = static_cast<int>(tg % groups);
        const int64_t row = (tg / groups) * 64 + lane;
        uint4 x = make_uint4(0, 0, 0, 0);
        if (row < n) {
            const int64_t o = perm[row];
            x = src[((o >> 6) * groups + gi) * 64 + (o & 63)];
        }
        dst[e] = x;
    }
}

}  // namespace vg

VG_API int32_t vg_vamana_reorder_bfs(vg_index *idx, uint32_t *perm, uint32_t *inv_perm, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_vamana_reorder_bfs: NULL index");
    VG_CHECK(idx->d_vamana || (idx->n == 0 && idx->vamana_r > 0), VG_ERR_NOT_READY, "vg_vamana_reorder_bfs: index has no Vamana graph");
    VG_CHECK(!idx->d_hnsw_l0 && !idx->d_hnsw_tomb && !idx->d_hnsw_l0_dist && !idx->d_centroids && idx->num_partitions == 0,
             VG_ERR_UNSUPPORTED,
             "vg_vamana_reorder_bfs: the index holds %s, state of a memtable or flat segment that the DiskANN writer never has",
             idx->d_hnsw_l0 ? "an HNSW graph" : idx->d_hnsw_tomb ? "HNSW tombstones" : idx->d_hnsw_l0_dist ? "HNSW edge distances"
                                                                                             : "IVF partitions");
    const int64_t n = idx->n;
    if (n == 0) return VG_OK;
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int r = idx->vamana_r;
    const uint32_t nn = static_cast<uint32_t>(n);

    // the arrays to permute, and the one scratch buffer: the largest of them
    const int64_t bf16_bytes = static_cast<int64_t>(idx->vectors_bf16_dim) * 2;
    const int64_t pq_m = idx->pq ? idx->pq->m : 0;
    const int64_t rq_nb = idx->d_rq_rows ? static_cast<int64_t>((idx->dim + 63) / 64 * 8) : 0;  // sign bytes (rq_words * 8)
    const int64_t int4_row = idx->d_int4_rows ? vg_int4_code_bytes(idx->dim) : 0;
    int64_t scratch_bytes = static_cast<int64_t>(n) * r * 4;
    auto need = [&](const void *p, int64_t bytes) {
        if (p) scratch_bytes = std::max(scratch_bytes, bytes);
    };
    need(idx->d_vectors, n * idx->dim * 4);
    need(idx->d_vectors_bf16, n * bf16_bytes);
    need(idx->d_pq_rows, n * pq_m);
    need(idx->pq_nom.row_image(), n * idx->pq_nom.dim_pad * 2);
    need(idx->d_rq_rows, n * (rq_nb + 4));
    need(idx->d_sq_tiles, idx->n_tiles * idx->sq_groups * 64 * 16);
    need(idx->sq_nom.row_image(), n * idx->sq_nom.dim_pad * 2);
    need(idx->d_int4_rows, n * int4_row);

    // BFS state: order (perm), inv (inv_perm), the large levels' keys, masks and counts, and the scratch
    vg::DevTmp<uint32_t> order, inv, counts;
    vg::DevTmp<unsigned long long> keys, masks;
    vg::DevTmp<vg::RbState> state;
    VG_TRY(order.init(n, st));
    VG_TRY(inv.init(n, st));
    VG_TRY(counts.init(n, st));
    VG_TRY(keys.init(n, st));
    VG_TRY(masks.init(n, st));
    VG_TRY(state.init(1, st));
    void *scratch = nullptr;
    VG_HIP(hipMalloc(&scratch, static_cast<size_t>(scratch_bytes)));
    struct Free {
        void *p;
        ~Free() { (void)hipFree(p); }
    } free_scratch{scratch};

    VG_HIP(hipMemsetAsync(inv.ptr, 0xFF, static_cast<size_t>(n) * 4, st));
    VG_HIP(hipMemsetAsync(keys.ptr, 0xFF, static_cast<size_t>(n) * 8, st));
    VG_HIP(hipMemsetAsync(state.ptr, 0, sizeof(vg::RbState), st));
    vg::RbState hs{};
    {
        vg::ProfScope prof(idx->ctx, "vamana_reorder_bfs", st);
        for (;;) {
            VG_LAUNCH(vg::rb_small_kernel, dim3(1), dim3(vg::kRbThreads), 0, st, idx->d_vamana, r, nn, idx->vamana_entry, order.ptr,
                      inv.ptr, state.ptr);
            VG_HIP(hipMemcpyAsync(&hs, state.ptr, sizeof(hs), hipMemcpyDeviceToHost, st));
            VG_HIP(hipStreamSynchronize(st));
            if (hs.lo == hs.hi) break;  // every id placed
            const uint32_t S = hs.hi - hs.lo;
            const unsigned blocks = (S + 3) / 4;
            VG_LAUNCH(vg::rb_discover_kernel, dim3(blocks), dim3(256), 0, st, idx->d_vamana, r, nn, order.ptr, hs.lo, S, inv.ptr, keys.ptr);
            VG_LAUNCH(vg::rb_mark_kernel, dim3(blocks), dim3(256), 0, st, idx->d_vamana, r, nn, order.ptr, hs.lo, S, inv.ptr, keys.ptr,
                      masks.ptr, counts.ptr);
            VG_LAUNCH(vg::rb_scan_kernel, dim3(1), dim3(vg::kRbThreads), 0, st, counts.ptr, S, state.ptr);
            VG_LAUNCH(vg::rb_place_kernel, dim3(blocks), dim3(256), 0, st, idx->d_vamana, r, order.ptr, hs.lo, S, hs.hi, inv.ptr, masks.ptr,
                      counts.ptr);
        }
    }
    VG_CHECK(hs.hi == nn, VG_ERR_HIP, "vg_vamana_reorder_bfs: the BFS placed %u of %u nodes", hs.hi, nn);

    {
        vg::ProfScope prof(idx->ctx, "vamana_reorder_permute", st);
        const uint32_t *p = order.ptr;
        // graph rows, ids through inv_perm
        if (r % 4 == 0)
            VG_LAUNCH(vg::rb_graph_kernel<true>, dim3(vg::rb_grid(n * r / 4)), dim3(256), 0, st, idx->d_vamana,
                      static_cast<uint32_t *>(scratch), n, r, p, inv.ptr);
        else
            VG_LAUNCH(vg::rb_graph_kernel<false>, dim3(vg::rb_grid(n * r)), dim3(256), 0, st, idx->d_vamana,
                      static_cast<uint32_t *>(scratch), n, r, p, inv.ptr);
        VG_HIP(hipMemcpyAsync(idx->d_vamana, scratch, static_cast<size_t>(n) * r * 4, hipMemcpyDeviceToDevice, st));
        // fp32 rows and their norms, the bf16 filter image
        VG_TRY(vg::rb_permute_rows(idx->d_vectors, n, static_cast<int64_t>(idx->dim) * 4, p, scratch, st));
        VG_TRY(vg::rb_permute_rows(idx->d_norms, n, 4, p, scratch, st));
        VG_TRY(vg::rb_permute_rows(idx->d_vectors_bf16, n, bf16_bytes, p, scratch, st));
        // PQ: the row-major codes, the tiles rebuilt from them, the nomination image and its norms
        if (idx->d_pq_rows) {
            VG_TRY(vg::rb_permute_rows(idx->d_pq_rows, n, pq_m, p, scratch, st));
            if (idx->d_pq_tiles)
                VG_TRY(vg::launch_pq_retile(idx->d_pq_rows, n, idx->pq->m, idx->pq_groups, (n + 63) / 64, idx->d_pq_tiles, st));
        }
        // (from the codes: no row image; its sample tiles are decoded per call)
        VG_TRY(vg::rb_permute_rows(idx->pq_nom.row_image(), n, static_cast<int64_t>(idx->pq_nom.dim_pad) * 2, p, scratch, st));
        VG_TRY(vg::rb_permute_rows(idx->pq_nom.norms, n, 4, p, scratch, st));
        // RaBitQ: rows, then tiles and norms[0, n) rebuilt from them (norms[n], the largest |norm|, does not move)
        if (idx->d_rq_rows) {
            VG_TRY(vg::rb_permute_rows(idx->d_rq_rows, n, rq_nb + 4, p, scratch, st));
            if (idx->d_rq_tiles)
                VG_TRY(vg::launch_rabitq_retile(idx->d_rq_rows, n, static_cast<int>(rq_nb), idx->rq_groups, (n + 63) / 64, idx->d_rq_tiles,
                                                idx->d_rq_norms, st));
        }
        // SQ8: the tiles piece by piece, the nomination image and its norms
        if (idx->d_sq_tiles) {
            const int64_t tiles = (n + 63) / 64;
            VG_LAUNCH(vg::rb_tiles_kernel, dim3(vg::rb_grid(tiles * idx->sq_groups * 64)), dim3(256), 0, st,
                      reinterpret_cast<const uint4 *>(idx->d_sq_tiles), static_cast<uint4 *>(scratch), n, idx->sq_groups, tiles, p);
            VG_HIP(hipMemcpyAsync(idx->d_sq_tiles, scratch, static_cast<size_t>(tiles * idx->sq_groups * 64 * 16), hipMemcpyDeviceToDevice,
                                  st));
        }
        // (from the codes: no row image, the norms alone move with the codes)
        VG_TRY(vg::rb_permute_rows(idx->sq_nom.row_image(), n, static_cast<int64_t>(idx->sq_nom.dim_pad) * 2, p, scratch, st));
        VG_TRY(vg::rb_permute_rows(idx->sq_nom.norms, n, 4, p, scratch, st));
        // INT4 rows
        VG_TRY(vg::rb_permute_rows(idx->d_int4_rows, n, int4_row, p, scratch, st));
    }
    if (perm) VG_HIP(hipMemcpyAsync(perm, order.ptr, static_cast<size_t>(n) * 4, hipMemcpyDefault, st));
    if (inv_perm) VG_HIP(hipMemcpyAsync(inv_perm, inv.ptr, static_cast<size_t>(n) * 4, hipMemcpyDefault, st));
    VG_HIP(hipStreamSynchronize(st));
    idx->vamana_entry = 0;  // inv_perm[entry]: the main BFS starts at the entry point
    return VG_OK;
}
