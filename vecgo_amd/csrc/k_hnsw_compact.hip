// k_hnsw_compact.hip — HNSW.Compact (internal/hnsw/compact.go:16-34) on a resident graph: repairActiveNodes /
// reconcileNode (:36-81, :174-233), pruneNodeConnections (:370-401), clearNodeConnections (:404-421).
//
//   compact_scan_kernel     checkRepairNeeded (:332-367): one lane per (level, node); a live node's list with fewer than M/2
//                           (layer 0: M) live members sets the level's bit in need[node].  The set of nodes to repair is fixed
//                           here, up front: a repair writes only its own node's lists, so no repair changes another node's
//                           answer.  The host reads need[] and lists the nodes in id order.
//   compact_repair_kernel   one wavefront per node to repair, batches of max_batch nodes: greedyDescent (:235-258) to the
//                           node's level, then per level that needs repair searchLayerPredicateAware (hnsw.go:1406-1557) on
//                           THAT level's lists with the filter "id != self" and the tombstones as isDeleted (the loop of
//                           k_hnsw_predicate.hip, which walks layer 0 under a bitmap), mergeCandidatesWithActiveNeighbors
//                           (:260-287) and updateConnectionsForRepair (:289-328) with selectNeighbors' heap drain replayed.
//                           The new list goes to a staging row; nothing is written under a running walk.
//   compact_apply_kernel    the batch's staged lists into the level tables (setConnections: ids and Neighbor.Dist).
//   compact_prune_kernel    phases 2 and 3 in one pass, one wavefront per (level, node): a live node's list loses its
//                           tombstoned ids (survivors keep order and cached distance), a tombstoned node's lists are emptied.
//                           One kernel because the two phases write disjoint rows (live owners / dead owners) and read only
//                           the row itself and the tombstones: no order between them can be observed.
//
// Levels the reference walks without effect are skipped.  reconcileNode walks and merges EVERY level from the node's level down,
// but a level that needs no repair leaves nothing behind: searchLayer starts with initializeSearch (hnsw.go:1567-1572: visited
// set and both queues reset), its entry (currID, currDist) is never updated (:226-231), the graph is only read, and the merged
// heap is s.Candidates, reset by the next level's initializeSearch.  So the levels that need repair are independent of the rest.
//
// The navigation queue is unbounded in the reference.  Here it has one slot per row (n + 1): a node is pushed at most once — the
// entry point, then only nodes whose visited bit was clear — so it cannot overflow and nothing is truncated.
#include <algorithm>
#include <vector>

#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_heap.hpp"
#include "vg_hnsw_layer.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"

namespace vg {

constexpr int kCompactMaxEf = 1024;    // the build's limit: results heap, merged set and drained list live in LDS
constexpr int kCompactLdsCand = 1024;  // navigation-heap items kept in LDS (the rest in HBM scratch), as the predicate walk
constexpr int kStage = 64;             // slots per staging row (M0 <= 64)

// The index's level tables with the Neighbor.Dist of every slot
struct CompactGraph {
    const float *base;
    int64_t n;
    int dim, metric, m0, m, max_level;
    uint32_t *l0;   // n * m0
    float *d0;      // n * m0 cached distances
    uint32_t *adj;  // upper rows * m
    float *du;      // upper rows * m cached distances
    const uint32_t *slots;
    const int64_t *level_off;
    const uint8_t *tomb;  // never null here
};

// first slot of node's list on `level` in (l0, d0) or (adj, du); -1: the node has no row on that level
__device__ __forceinline__ int64_t cg_off(const CompactGraph &g, uint32_t node, int level)
{
    if (level == 0) return static_cast<int64_t>(node) * g.m0;
    const uint32_t slot = g.slots[static_cast<int64_t>(level - 1) * g.n + node];
    return slot == VG_INVALID_ID ? -1 : (g.level_off[level - 1] + slot) * g.m;
}
__device__ __forceinline__ uint32_t *cg_ids(const CompactGraph &g, int level) { return level == 0 ? g.l0 : g.adj; }
__device__ __forceinline__ float *cg_dist(const CompactGraph &g, int level) { return level == 0 ? g.d0 : g.du; }
__device__ __forceinline__ bool cg_dead(const CompactGraph &g, uint32_t id) { return (g.tomb[id >> 3] >> (id & 7)) & 1; }

// Neighbor.Dist of the upper levels' slots by the pair kernel (a graph the index did not build keeps none): what
// hnsw_edge_dist_kernel is to layer 0.  One wavefront per (level >= 1, node).
__global__ __launch_bounds__(64) void compact_upper_dist_kernel(CompactGraph g)
{
    __shared__ float nb_pair[64], nb_bnd[64];
    const int lane = threadIdx.x;
    const int64_t total = static_cast<int64_t>(g.max_level) * g.n;
    for (int64_t e = blockIdx.x; e < total; e += gridDim.x) {
        const int level = static_cast<int>(e / g.n) + 1;
        const uint32_t node = static_cast<uint32_t>(e - static_cast<int64_t>(level - 1) * g.n);
        const int64_t off = cg_off(g, node, level);
        if (off < 0) continue;
        F32Scorer sc;
        sc.base = g.base;
        sc.qv = g.base + static_cast<int64_t>(node) * g.dim;
        sc.dim = g.dim;
        sc.metric = g.metric;
        sc.sub = Sub16::make(lane);
        const uint32_t id_lane = lane < g.m ? g.adj[off + lane] : VG_INVALID_ID;
        const uint64_t inval = __ballot(id_lane == VG_INVALID_ID);
        const int count = inval ? __builtin_ctzll(inval) : 64;
        const uint64_t mask = count >= 64 ? ~0ull : ((1ull << count) - 1);
        sc.many(mask, id_lane, lane, nb_pair, nb_bnd);
        __syncthreads();
        if (lane < g.m) g.du[off + lane] = lane < count ? nb_pair[lane] : 0.0f;
        __syncthreads();
    }
}

// checkRepairNeeded (compact.go:332-367), one lane per (level, node)
__global__ void compact_scan_kernel(CompactGraph g, unsigned long long *__restrict__ need)
{
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= static_cast<int64_t>(g.max_level + 1) * g.n) return;
    const int level = static_cast<int>(e / g.n);
    const uint32_t node = static_cast<uint32_t>(e - static_cast<int64_t>(level) * g.n);
    if (cg_dead(g, node)) return;
    const int64_t off = cg_off(g, node, level);
    if (off < 0) return;
    const uint32_t *ids = cg_ids(g, level) + off;
    const int deg = level == 0 ? g.m0 : g.m;
    int active = 0;
    for (int i = 0; i < deg; i++) {
        const uint32_t id = ids[i];
        if (id == VG_INVALID_ID) break;
        active += cg_dead(g, id) ? 0 : 1;
    }
    const int threshold = level == 0 ? g.m : g.m / 2;
    if (active < threshold) atomicOr(&need[node], 1ull << level);
}

// ---- phase 1 ----------------------------------------------------------------------------------------------------------
// rep[b0 + i], i < bcount: the batch's nodes; pair_base[i]: index of rep[i]'s first (node, level) pair among the call's,
// a node's pairs in the order its levels are repaired (top down); staging rows are relative to pair_base[b0].
__global__ __launch_bounds__(64) void compact_repair_kernel(CompactGraph g, uint32_t entry, const uint32_t *__restrict__ rep,
                                                            const unsigned long long *__restrict__ need,
                                                            const int64_t *__restrict__ pair_base, int64_t b0, int64_t bcount, int ef,
                                                            int n2_max, uint32_t *__restrict__ visited_ws, int64_t vis_words,
                                                            HItem *__restrict__ cand_ws, int64_t cand_cap, uint32_t *__restrict__ st_ids,
                                                            float *__restrict__ st_dist, int32_t *__restrict__ st_cnt,
                                                            uint32_t *__restrict__ st_node, int32_t *__restrict__ st_level)
{
    extern __shared__ __attribute__((aligned(8))) unsigned char smem[];
    float *nb_pair = reinterpret_cast<float *>(smem);
    float *nb_bnd = nb_pair + 64;
    uint32_t *fin_id = reinterpret_cast<uint32_t *>(nb_bnd + 64);
    float *fin_d = reinterpret_cast<float *>(fin_id + 64);
    HItem *cand_lo = reinterpret_cast<HItem *>(fin_d + 64);  // the walk's navigation heap; afterwards the drained list
    HItem *res = cand_lo + kCompactLdsCand;                  // ef + 1 items: the walk's results; afterwards the merged heap
    uint64_t *keys = reinterpret_cast<uint64_t *>(res + ((ef + 2) & ~1));  // n2_max keys: the merged set, by id
    const int lane = threadIdx.x;
    uint32_t *vis = visited_ws + static_cast<int64_t>(blockIdx.x) * vis_words;
    HItem *cand_lo_flat = cand_lo;  // (see vamana_search_kernel: the flat LDS address has to pass through a register)
    asm volatile("" : "+s"(cand_lo_flat));
    const SplitHeap cand{cand_lo_flat, cand_ws + static_cast<int64_t>(blockIdx.x) * cand_cap, kCompactLdsCand};
    const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));

    for (int64_t bi = blockIdx.x; bi < bcount; bi += gridDim.x) {
        const uint32_t self = rep[b0 + bi];
        const unsigned long long levels = need[self];
        int node_level = 0;
        for (int l = g.max_level; l >= 1; l--)
            if (g.slots[static_cast<int64_t>(l - 1) * g.n + self] != VG_INVALID_ID) {
                node_level = l;
                break;
            }
        F32Scorer sc;
        sc.base = g.base;
        sc.qv = g.base + static_cast<int64_t>(self) * g.dim;
        sc.dim = g.dim;
        sc.metric = g.metric;
        sc.sub = Sub16::make(lane);

        // greedyDescent (compact.go:235-258): the shape of greedySearch; tombstoned nodes are walked like any other
        uint32_t cur = entry;
        float cur_d = sc.one(cur);
        for (int level = g.max_level; level > node_level; level--) {
            auto row_of = [&](uint32_t node) -> const uint32_t * {
                const int64_t off = cg_off(g, node, level);
                return off < 0 ? nullptr : g.adj + off;
            };
            greedy_layer(sc, lane, row_of, g.m, nb_pair, nb_bnd, cur, cur_d);
        }

        int64_t p = pair_base[b0 + bi] - pair_base[b0];
        for (int level = node_level; level >= 0; level--) {
            if (!((levels >> level) & 1)) continue;
            const int deg = level == 0 ? g.m0 : g.m;
            const uint32_t *lids = cg_ids(g, level);
            const float *ldist = cg_dist(g, level);
            for (int64_t w = lane; w < vis_words; w += 64) vis[w] = 0;  // initializeSearch: Visited.Reset()
            __threadfence();
            __syncthreads();

            // ---- searchLayerPredicateAware from (cur, cur_d), never updated (compact.go:226-231); filter: id != self ----
            int cand_len = 0, res_len = 0;
            if (lane == 0) atomicOr(&vis[cur >> 5], 1u << (cur & 31));
            heap_push<false>(cand, cand_len, HItem{cur, cur_d});
            if (cur != self && !cg_dead(g, cur)) heap_push<true>(res, res_len, HItem{cur, cur_d});
            int misses = 0;  // consecutiveFilterMisses
            __syncthreads();
            while (cand_len > 0) {
                const HItem c = heap_pop<false>(cand, cand_len);
                if (res_len >= ef && c.dist > heap_get(res, 0).dist) break;
                const int64_t off = cg_off(g, c.node, level);
                const uint32_t id_lane = (off >= 0 && lane < deg) ? lids[off + lane] : VG_INVALID_ID;
                const float edge_lane = (off >= 0 && lane < deg) ? ldist[off + lane] : 0.0f;
                const uint64_t inval = __ballot(id_lane == VG_INVALID_ID);
                const int count = inval ? __builtin_ctzll(inval) : 64;
                bool fresh = false;
                if (lane < count) {  // CheckAndVisit for the whole list (a node's neighbour ids are distinct)
                    const uint32_t bit = 1u << (id_lane & 31);
                    fresh = (atomicOr(&vis[id_lane >> 5], bit) & bit) == 0;
                }
                const uint64_t newmask = __ballot(fresh);
                if (!newmask) continue;
                const bool passes = fresh && id_lane != self;
                const bool dead = fresh && cg_dead(g, id_lane);
                const uint64_t passmask = __ballot(passes), livemask = __ballot(passes && !dead);
                // as in hnsw_predicate_kernel: the passing live nodes are scored together ahead of the replay, a rejected
                // node only where the replay reaches a branch that computes its distance
                sc.many(livemask, id_lane, lane, nb_pair, nb_bnd);
                __syncthreads();
                float my_d = nb_pair[lane];
                bool rej_scored = false;
                auto rejected_dist = [&](int j) {
                    if (!rej_scored) {
                        sc.many(newmask & ~livemask & ~((1ull << j) - 1), id_lane, lane, nb_pair, nb_bnd);
                        __syncthreads();
                        my_d = nb_pair[lane];
                        rej_scored = true;
                    }
                    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_d), j));
                };
                uint64_t todo = newmask;
                while (todo) {
                    const int j = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const bool pj = (passmask >> j) & 1, live = (livemask >> j) & 1;
                    misses = pj ? 0 : misses + 1;
                    const uint32_t id = static_cast<uint32_t>(__builtin_amdgcn_readlane(id_lane, j));
                    float nd;
                    if (live) {
                        nd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_d), j));
                    } else if (res_len < ef / 2) {
                        const float edge = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(edge_lane), j));
                        nd = edge > 0.0f ? edge : rejected_dist(j);
                    } else if (res_len < ef) {
                        if (misses > 10) continue;  // filterMissGateThreshold
                        const float edge = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(edge_lane), j));
                        if (edge > 0.0f && res_len > 0 && edge > heap_get(res, 0).dist * 1.5f) continue;
                        nd = rejected_dist(j);
                    } else {
                        continue;
                    }
                    if (res_len >= ef && nd > heap_get(res, 0).dist) continue;  // shouldExplore
                    if (cand_len >= cand_cap) continue;  // (unreachable: one slot per row, a node is pushed at most once)
                    heap_push<false>(cand, cand_len, HItem{id, nd});
                    if (live) res_push_bounded<false>(res, res_len, HItem{id, nd}, ef);
                }
                __syncthreads();
            }
            __syncthreads();

            // ---- mergeCandidatesWithActiveNeighbors (compact.go:260-287) ----
            // the map: the walk's results (their ids are distinct), then the node's live neighbours — a new id is added, a
            // present one keeps the smaller distance (`<`); pushed back in ascending id order (the rule the reference's map
            // order leaves open) with PushItemBounded(EF)
            const int64_t own = cg_off(g, self, level);  // the node has this level: its bit was set from this row
            const uint32_t oid = lane < deg ? lids[own + lane] : VG_INVALID_ID;
            const float od = lane < deg ? ldist[own + lane] : 0.0f;
            const uint64_t oinval = __ballot(oid == VG_INVALID_ID);
            const int ocount = oinval ? __builtin_ctzll(oinval) : 64;
            const bool own_dead = lane < ocount && cg_dead(g, oid);
            const bool own_live = lane < ocount && !own_dead;
            const uint64_t deadmask = __ballot(own_dead);
            const int kept = __popcll(deadmask);
            int found = -1;
            for (int i = 0; i < res_len; i++)
                if (own_live && res[i].node == oid) found = i;
            if (found >= 0 && od < res[found].dist) res[found].dist = od;
            const uint64_t addmask = __ballot(own_live && found < 0);
            const int total = res_len + __popcll(addmask);
            int n2 = 64;
            while (n2 < total) n2 <<= 1;  // <= n2_max: total <= ef + M0
            __syncthreads();
            for (int i = lane; i < n2; i += 64)
                keys[i] = i < res_len ? (static_cast<uint64_t>(res[i].node) << 32) | __float_as_uint(res[i].dist) : kKeyMax;
            __syncthreads();
            if (own_live && found < 0) keys[res_len + __popcll(addmask & lt_mask)] = (static_cast<uint64_t>(oid) << 32) | __float_as_uint(od);
            __syncthreads();
            bitonic_sort_lds(keys, n2, lane, 64);
            int heap_len = 0;
            for (int i = 0; i < total; i++) {
                const uint64_t key = keys[i];
                res_push_bounded<false>(res, heap_len, HItem{static_cast<uint32_t>(key >> 32), __uint_as_float(static_cast<uint32_t>(key))}, ef);
            }

            // ---- updateConnectionsForRepair (compact.go:289-328) ----
            // selectNeighbors (hnsw.go:986-1106) over the merged heap: the drain, nearest first, then the heuristic and the fill-up
            const int want = deg - kept > 0 ? deg - kept : 0;  // numToSelect
            const int nc = heap_len;
            for (int i = nc - 1; i >= 0; i--) heap_put(cand_lo, i, heap_pop<true>(res, heap_len));
            __syncthreads();
            int nsel = 0;
            uint32_t sel_id = VG_INVALID_ID;  // lane s: the s-th selected item
            float sel_d = 0.0f;
            if (nc <= want) {  // selectNeighborsSimple: everything
                if (lane < nc) {
                    const HItem it = heap_get(cand_lo, lane);
                    sel_id = it.node;
                    sel_d = it.dist;
                }
                nsel = nc;
            } else {
                F32Scorer pc = sc;
                for (int i = 0; i < nc && nsel < want; i++) {  // applyHeuristic
                    const HItem cd = heap_get(cand_lo, i);
                    uint64_t closer = 0;
                    if (nsel > 0) {
                        pc.qv = g.base + static_cast<int64_t>(cd.node) * g.dim;
                        pc.many(nsel >= 64 ? ~0ull : ((1ull << nsel) - 1), sel_id, lane, nb_pair, nb_bnd);
                        __syncthreads();
                        closer = __ballot(lane < nsel && nb_pair[lane] < cd.dist);
                        __syncthreads();
                    }
                    if (closer) continue;
                    if (lane == nsel) {
                        sel_id = cd.node;
                        sel_d = cd.dist;
                    }
                    nsel++;
                }
                for (int i = 0; i < nc && nsel < want; i++) {  // fillUpNeighbors
                    const HItem cd = heap_get(cand_lo, i);
                    if (__ballot(lane < nsel && sel_id == cd.node)) continue;
                    if (lane == nsel) {
                        sel_id = cd.node;
                        sel_d = cd.dist;
                    }
                    nsel++;
                }
            }
            // the list: the kept tombstones in slot order, then the selected items — only if something was selected (:315)
            fin_id[lane] = VG_INVALID_ID;
            fin_d[lane] = 0.0f;
            __syncthreads();
            if (own_dead) {
                const int at = __popcll(deadmask & lt_mask);
                fin_id[at] = oid;
                fin_d[at] = od;
            }
            if (lane < nsel) {
                fin_id[kept + lane] = sel_id;
                fin_d[kept + lane] = sel_d;
            }
            __syncthreads();
            st_ids[p * kStage + lane] = fin_id[lane];
            st_dist[p * kStage + lane] = fin_d[lane];
            if (lane == 0) {
                st_cnt[p] = nsel > 0 ? kept + nsel : -1;
                st_node[p] = self;
                st_level[p] = level;
            }
            __syncthreads();
            p++;
        }
    }
}

// setConnections of a batch's repaired lists; counters[1] counts them
__global__ __launch_bounds__(64) void compact_apply_kernel(CompactGraph g, const uint32_t *__restrict__ st_ids, const float *__restrict__ st_dist,
                                                           const int32_t *__restrict__ st_cnt, const uint32_t *__restrict__ st_node,
                                                           const int32_t *__restrict__ st_level, unsigned long long *__restrict__ counters)
{
    const int64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    if (st_cnt[p] < 0) return;
    const int level = st_level[p];
    const int64_t off = cg_off(g, st_node[p], level);
    const int deg = level == 0 ? g.m0 : g.m;
    if (lane < deg) {
        cg_ids(g, level)[off + lane] = st_ids[p * kStage + lane];
        cg_dist(g, level)[off + lane] = st_dist[p * kStage + lane];
    }
    if (lane == 0) atomicAdd(&counters[1], 1ull);
}

// ---- phases 2 and 3 -----------------------------------------------------------------------------------------------------
// One wavefront per (level, node), lane = slot: every lane has read its slot before any lane writes one.  A tombstoned node
// is handled once, by its layer-0 wavefront, over all its levels (counters[3] counts it if any of its lists held a link).
__global__ __launch_bounds__(256) void compact_prune_kernel(CompactGraph g, unsigned long long *__restrict__ counters)
{
    const int lane = threadIdx.x & 63;
    const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int64_t total = static_cast<int64_t>(g.max_level + 1) * g.n;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 4;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); e < total; e += stride) {
        const int level = static_cast<int>(e / g.n);
        const uint32_t node = static_cast<uint32_t>(e - static_cast<int64_t>(level) * g.n);
        if (cg_dead(g, node)) {  // clearNodeConnections (compact.go:404-421): no exception for the entry point
            if (level > 0) continue;
            bool any = false;
            for (int l = 0; l <= g.max_level; l++) {
                const int64_t off = cg_off(g, node, l);
                if (off < 0) break;  // a node's levels are 0 .. its level
                const int deg = l == 0 ? g.m0 : g.m;
                if (__ballot(lane < deg && cg_ids(g, l)[off + lane] != VG_INVALID_ID)) any = true;
                if (lane < deg) {
                    cg_ids(g, l)[off + lane] = VG_INVALID_ID;
                    cg_dist(g, l)[off + lane] = 0.0f;
                }
            }
            if (any && lane == 0) atomicAdd(&counters[3], 1ull);
            continue;
        }
        const int64_t off = cg_off(g, node, level);  // pruneNodeConnections (compact.go:370-401)
        if (off < 0) continue;
        const int deg = level == 0 ? g.m0 : g.m;
        uint32_t *ids = cg_ids(g, level) + off;
        float *dist = cg_dist(g, level) + off;
        const uint32_t id = lane < deg ? ids[lane] : VG_INVALID_ID;
        const float d = lane < deg ? dist[lane] : 0.0f;
        const uint64_t inval = __ballot(id == VG_INVALID_ID);
        const int count = inval ? __builtin_ctzll(inval) : 64;
        const bool dead = lane < count && cg_dead(g, id);
        const uint64_t deadmask = __ballot(dead), keepmask = __ballot(lane < count && !dead);
        if (!deadmask) continue;  // hasTombstones
        const int nkeep = __popcll(keepmask);
        if (lane < count && !dead) {
            const int at = __popcll(keepmask & lt_mask);
            ids[at] = id;
            dist[at] = d;
        }
        if (lane >= nkeep && lane < deg) {
            ids[lane] = VG_INVALID_ID;
            dist[lane] = 0.0f;
        }
        if (lane == 0) atomicAdd(&counters[2], static_cast<unsigned long long>(__popcll(deadmask)));
    }
}

}  // namespace vg

VG_API int32_t vg_hnsw_compact(vg_index *idx, int32_t ef_construction, int32_t max_batch, vg_hnsw_compact_stats *stats, void *stream)
{
    const char *fn = "vg_hnsw_compact";
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(idx->d_hnsw_l0, VG_ERR_NOT_READY, "%s: index has no HNSW graph", fn);
    VG_CHECK(idx->d_vectors, VG_ERR_NOT_READY, "%s: index has no fp32 vectors", fn);
    VG_CHECK(max_batch >= 1, VG_ERR_INVALID_ARG, "%s: max_batch must be >= 1", fn);
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    if (ef_construction == 0) ef_construction = 300;  // Options.EF hnsw.go:37
    VG_CHECK(ef_construction >= 1 && ef_construction <= vg::kCompactMaxEf, VG_ERR_UNSUPPORTED,
             "%s: ef_construction=%d must be in 1..%d (0 = 300)", fn, ef_construction, vg::kCompactMaxEf);
    const int m = idx->hnsw_m, m0 = idx->hnsw_m0;
    VG_CHECK(m >= 2 && m <= 32 && m0 == 2 * m, VG_ERR_UNSUPPORTED, "%s: the graph's M=%d, M0=%d: M must be in 2..32 and M0 = 2M", fn, m, m0);
    const char *held = vg::held_segment_state(idx);
    VG_CHECK(!held, VG_ERR_UNSUPPORTED, "%s: the index holds %s (segment state, not a memtable's)", fn, held);
    VG_CHECK(idx->hnsw_max_level < 63, VG_ERR_UNSUPPORTED, "%s: %d levels (at most 63)", fn, idx->hnsw_max_level + 1);
    if (stats) *stats = vg_hnsw_compact_stats{0, 0, 0, 0};
    const int64_t n = idx->n;
    if (!idx->d_hnsw_tomb || n == 0) return VG_OK;
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int ef = ef_construction;
    const int L = idx->hnsw_max_level;

    std::vector<uint8_t> tomb(static_cast<size_t>((n + 7) / 8));
    VG_HIP(hipMemcpyAsync(tomb.data(), idx->d_hnsw_tomb, tomb.size(), hipMemcpyDeviceToHost, st));
    std::vector<int64_t> level_off(static_cast<size_t>(L) + 1, 0);
    if (L > 0) VG_HIP(hipMemcpyAsync(level_off.data(), idx->d_hnsw_level_off, level_off.size() * 8, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    if (n & 7) tomb.back() &= static_cast<uint8_t>((1u << (n & 7)) - 1);
    if (std::all_of(tomb.begin(), tomb.end(), [](uint8_t b) { return b == 0; })) return VG_OK;
    const int64_t upper_rows = level_off[static_cast<size_t>(L)];

    // Neighbor.Dist of every slot: vg_hnsw_insert's rule.  A graph the index built or grew: its cached distances, rewritten in
    // place with the lists.  An uploaded graph: layer 0 = the edge distances of vg_index_set_hnsw_edge_distances (computed by
    // the pair kernel when there are none), rewritten in place; upper levels = the pair kernel's, for this call only.
    const bool built = idx->d_hnsw_l0_cdist && (L == 0 || idx->d_hnsw_adj_cdist);
    vg::DevTmp<float> upper_dist;
    vg::CompactGraph g{idx->d_vectors, n, idx->dim, idx->metric, m0, m, L, idx->d_hnsw_l0, nullptr, idx->d_hnsw_adj, nullptr,
                       idx->d_hnsw_slot, idx->d_hnsw_level_off, idx->d_hnsw_tomb};
    const unsigned wave_blocks = static_cast<unsigned>(std::min<int64_t>(n, int64_t(idx->ctx->compute_units) * 64));
    if (built) {
        g.d0 = idx->d_hnsw_l0_cdist;
        g.du = idx->d_hnsw_adj_cdist;
    } else {
        if (!idx->d_hnsw_l0_dist) VG_TRY(vg::hnsw_edge_distances(idx, nullptr, st));
        g.d0 = idx->d_hnsw_l0_dist;
        VG_TRY(upper_dist.init(static_cast<size_t>(upper_rows) * m, st));
        g.du = upper_dist.ptr;
        if (upper_rows > 0) {
            vg::ProfScope prof(idx->ctx, "hnsw_compact_upper_dist", st);
            VG_LAUNCH(vg::compact_upper_dist_kernel, dim3(wave_blocks), dim3(64), 0, st, g);
        }
    }

    // ---- which nodes, which levels ----
    vg::DevTmp<unsigned long long> need, counters;
    VG_TRY(need.init(static_cast<size_t>(n), st));
    VG_TRY(counters.init(4, st));
    VG_HIP(hipMemsetAsync(need.ptr, 0, static_cast<size_t>(n) * 8, st));
    VG_HIP(hipMemsetAsync(counters.ptr, 0, 4 * 8, st));
    {
        const int64_t pairs = static_cast<int64_t>(L + 1) * n;
        vg::ProfScope prof(idx->ctx, "hnsw_compact_scan", st);
        VG_LAUNCH(vg::compact_scan_kernel, dim3(static_cast<unsigned>((pairs + 255) / 256)), dim3(256), 0, st, g, need.ptr);
    }
    std::vector<unsigned long long> h_need(static_cast<size_t>(n));
    VG_HIP(hipMemcpyAsync(h_need.data(), need.ptr, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> rep;
    std::vector<int64_t> pair_base(1, 0);
    for (int64_t i = 0; i < n; i++)
        if (h_need[static_cast<size_t>(i)]) {
            rep.push_back(static_cast<uint32_t>(i));
            pair_base.push_back(pair_base.back() + __builtin_popcountll(h_need[static_cast<size_t>(i)]));
        }
    const int64_t nrep = static_cast<int64_t>(rep.size());

    // ---- phase 1: batches of max_batch nodes in id order, each over the graph as it stood when the batch began ----
    if (nrep > 0) {
        int64_t max_pairs = 1;
        for (int64_t b0 = 0; b0 < nrep; b0 += max_batch) {
            const int64_t b1 = std::min<int64_t>(nrep, b0 + max_batch);
            max_pairs = std::max(max_pairs, pair_base[static_cast<size_t>(b1)] - pair_base[static_cast<size_t>(b0)]);
        }
        const int64_t vis_words = (n + 31) / 32, cand_cap = n + 1;
        const int64_t per_wave = vis_words * 4 + cand_cap * static_cast<int64_t>(sizeof(vg::HItem));
        // as many waves as the scratch cap holds (a wave takes the batch's nodes in turn), at most 16 per compute unit
        const int64_t waves = std::max<int64_t>(1, std::min<int64_t>({std::min<int64_t>(nrep, max_batch), vg::scratch_cap(idx->ctx) / per_wave,
                                                                       int64_t(idx->ctx->compute_units) * 16}));
        int n2_max = 64;
        while (n2_max < ef + m0) n2_max <<= 1;
        vg::ArenaCall ar(idx->ctx, st);
        const int a_vis = ar.add(static_cast<size_t>(waves * vis_words) * 4), a_cand = ar.add(static_cast<size_t>(waves * cand_cap) * sizeof(vg::HItem)),
                  a_rep = ar.add(rep.size() * 4), a_pb = ar.add(pair_base.size() * 8),
                  a_sid = ar.add(static_cast<size_t>(max_pairs) * vg::kStage * 4), a_sd = ar.add(static_cast<size_t>(max_pairs) * vg::kStage * 4),
                  a_sc = ar.add(static_cast<size_t>(max_pairs) * 4), a_sn = ar.add(static_cast<size_t>(max_pairs) * 4),
                  a_sl = ar.add(static_cast<size_t>(max_pairs) * 4);
        VG_TRY(ar.commit());
        uint32_t *d_rep = ar.get<uint32_t>(a_rep);
        int64_t *d_pb = ar.get<int64_t>(a_pb);
        VG_HIP(hipMemcpyAsync(d_rep, rep.data(), rep.size() * 4, hipMemcpyHostToDevice, st));
        VG_HIP(hipMemcpyAsync(d_pb, pair_base.data(), pair_base.size() * 8, hipMemcpyHostToDevice, st));
        const size_t lds = 256 * sizeof(float) + sizeof(vg::HItem) * (vg::kCompactLdsCand + static_cast<size_t>((ef + 2) & ~1)) +
                           sizeof(uint64_t) * static_cast<size_t>(n2_max);
        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vg::compact_repair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(lds)));
        for (int64_t b0 = 0; b0 < nrep; b0 += max_batch) {
            const int64_t bcount = std::min<int64_t>(max_batch, nrep - b0);
            const int64_t bpairs = pair_base[static_cast<size_t>(b0 + bcount)] - pair_base[static_cast<size_t>(b0)];
            {
                vg::ProfScope prof(idx->ctx, "hnsw_compact_repair", st);
                VG_LAUNCH(vg::compact_repair_kernel, dim3(static_cast<unsigned>(std::min(waves, bcount))), dim3(64), lds, st, g, idx->hnsw_entry,
                          d_rep, need.ptr, d_pb, b0, bcount, ef, n2_max, ar.get<uint32_t>(a_vis), vis_words, ar.get<vg::HItem>(a_cand), cand_cap,
                          ar.get<uint32_t>(a_sid), ar.get<float>(a_sd), ar.get<int32_t>(a_sc), ar.get<uint32_t>(a_sn), ar.get<int32_t>(a_sl));
            }
            vg::ProfScope prof(idx->ctx, "hnsw_compact_apply", st);
            VG_LAUNCH(vg::compact_apply_kernel, dim3(static_cast<unsigned>(bpairs)), dim3(64), 0, st, g, ar.get<uint32_t>(a_sid),
                      ar.get<float>(a_sd), ar.get<int32_t>(a_sc), ar.get<uint32_t>(a_sn), ar.get<int32_t>(a_sl), counters.ptr);
        }
    }

    // ---- phases 2 and 3 ----
    {
        vg::ProfScope prof(idx->ctx, "hnsw_compact_prune", st);
        const int64_t pairs = static_cast<int64_t>(L + 1) * n;
        const unsigned blocks = static_cast<unsigned>(std::min<int64_t>((pairs + 3) / 4, int64_t(idx->ctx->compute_units) * 32));
        VG_LAUNCH(vg::compact_prune_kernel, dim3(blocks), dim3(256), 0, st, g, counters.ptr);
    }
    unsigned long long h_counters[4] = {0, 0, 0, 0};
    VG_HIP(hipMemcpyAsync(h_counters, counters.ptr, sizeof h_counters, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    if (built) {
        vg::drop_device(&idx->d_hnsw_l0_dist);  // recomputed from the rows for the old lists: dropped, as vg_hnsw_insert drops it
    } else {  // (a partial set: never read as the graph's)
        vg::drop_device(&idx->d_hnsw_l0_cdist);
        vg::drop_device(&idx->d_hnsw_adj_cdist);
    }
    if (stats) {
        stats->repaired_nodes = nrep;
        stats->repaired_lists = static_cast<int64_t>(h_counters[1]);
        stats->pruned_links = static_cast<int64_t>(h_counters[2]);
        stats->cleared_nodes = static_cast<int64_t>(h_counters[3]);
    }
    return VG_OK;
}
