// k_hnsw_build.hip — HNSW construction on the GPU: hnsw.go:713-984 (insert / insertNode), :986-1106
// (selectNeighbors*, applyHeuristic, fillUpNeighbors), :455-555 (addConnection*), :885-900
// (updateEntryPoint), with the ids and levels of ApplyInsert / ApplyBatchInsert (:629-684: ids are the
// row numbers, level = layerForApplyInsert(id) :2103-2116).
//
// Nodes are inserted in id order in batches; a batch is what ApplyBatchInsert's goroutines are to each
// other: every node of the batch searches the graph as it stood when the batch began, then the batch's
// links are applied in id order.  batch = clamp(inserted / growth_div, 1, max_batch); max_batch = 1 is the
// reference's sequential Insert loop.  Per batch:
//   1. build_search_kernel   one wavefront per new node: greedy descent above its level, then
//                            searchLayerUnfiltered(ef) on every level it owns (vg_hnsw_layer.hpp); the
//                            results heap is popped into a best-first candidate list per (node, level).
//   2. build_select_kernel   one workgroup per (node, level): selectNeighborsHeuristic over the list; the
//                            node's own row is written, and one back-link record per chosen neighbour.
//   3. the back-link records are grouped by target row (vg_group_records.hpp, build_fill_kernel);
//      build_link_kernel     one workgroup (4 waves) per target row applies its records in id order: append while
//                            the row has room (addConnectionSimple), else addConnectionPrune; the four waves share
//                            the 64 pair distances of a link, wave 0 keeps the row.
//
// What makes addConnectionPrune affordable: a row keeps, next to the ids and the cached distances the
// reference keeps (node.go Neighbor{ID, Dist}), a 64 x 64 BIT matrix: bit j of bits[i] = "d(c_i, c_j) <
// d(s, c_i)", the only thing applyHeuristic ever asks about a pair of candidates.  The reference recomputes
// ~2000 pair distances of 768 floats on every back link of a full row (64 back links per insert); here a
// back link costs the 64 distances between the new node and the row's members, the heuristic itself is a
// replay over bit masks.  Every distance is the reference's kernel in its summation order (vg_exact.hpp) and
// every candidate order is the order the reference's 4-ary heap would pop (rank by distance; on equal
// distances the heap is replayed in LDS), so the graph equals what a letter-by-letter CPU run of hnsw.go builds
// (the test oracle) — bit for bit, ties included.
//
// vg_hnsw_insert runs the same batches on a graph the index already holds: rows appended, the per-row build state of
// older rows derived on demand (build_derive_kernel), see the comments at the entry point and DESIGN.md "HNSW insert".
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "vg_build_plan.hpp"
#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_group_records.hpp"
#include "vg_grow_rows.hpp"
#include "vg_heap.hpp"
#include "vg_hnsw_layer.hpp"
#include "vg_internal.hpp"

namespace vg {

constexpr int kBuildMaxEf = 1024;   // candidates per (node, level); heaps of the insert search live in LDS
constexpr int kSelThreads = 256;

// The graph under construction.  Rows: layer 0 row of node i = i (m0 slots); the row of node i on level
// l >= 1 = n + level_off[l-1] + slots[(l-1)*n + i] (m slots).  The ids live in two tables: `ids` = the n*m0
// layer-0 slots (the l0 table of vg_index_set_hnsw_graph), `ids_up` = the upper levels' rows (its adj).  The
// build allocates them as one array (ids_up = ids + n*m0); vg_hnsw_insert links straight into the index's tables.
//
// Build state (dist, bits, cnt, good) is kept per STATE row.  The build makes every row itself and keeps state for
// all of them: state row = row (smap null).  vg_hnsw_insert keeps it only for the rows the call touches: smap[row] =
// the row's state row, -1 until the select kernel makes the row (a new node's row: state row = its pair index) or
// build_derive_kernel derives it from the graph (a row that existed before the call: state rows from npairs on).
struct BuildGraph {
    const float *base;
    int64_t n;
    int dim, metric, m0, m;
    uint32_t *ids;    // layer-0 rows; 0xFFFFFFFF beyond cnt
    uint32_t *ids_up; // upper rows
    float *dist;      // d(row's node, member) as the insert search computed it
    uint64_t *bits;   // bit j of bits[slot i]: d(member i, member j) < dist[i]
    int32_t *cnt;     // per state row
    uint8_t *good;    // per state row: full, and every member was CHOSEN by the heuristic (none filled up): see build_link_kernel
    const uint32_t *slots;
    const int64_t *level_off;
    int32_t *smap;      // vg_hnsw_insert: row -> state row (-1: none yet); null: the state row is the row
    uint32_t *srow_row; // vg_hnsw_insert: state row -> row
    uint32_t *row_node; // vg_hnsw_insert: the node of every row a back-link record targets (written by the select kernel)
};

__device__ __forceinline__ int64_t bg_row(const BuildGraph &g, uint32_t node, int level)
{
    if (level == 0) return node;
    return g.n + g.level_off[level - 1] + g.slots[static_cast<int64_t>(level - 1) * g.n + node];
}
__device__ __forceinline__ int64_t bg_off(const BuildGraph &g, int64_t row)
{
    return row < g.n ? row * g.m0 : g.n * g.m0 + (row - g.n) * g.m;
}
__device__ __forceinline__ int bg_deg(const BuildGraph &g, int64_t row) { return row < g.n ? g.m0 : g.m; }
__device__ __forceinline__ uint32_t *bg_ids(const BuildGraph &g, int64_t row)
{
    return row < g.n ? g.ids + row * g.m0 : g.ids_up + (row - g.n) * g.m;
}
constexpr int kStateStride = 64;  // slots per state row of vg_hnsw_insert (M0 <= 64)
// first slot of a state row in dist / bits
__device__ __forceinline__ int64_t bg_soff(const BuildGraph &g, int64_t row, int64_t srow)
{
    return g.smap ? srow * kStateStride : bg_off(g, row);
}

// h.distanceFunc (newDistanceFunc hnsw.go:2218-2238) of two rows, all lanes of the 16-lane group
__device__ __forceinline__ float bg_pair(const BuildGraph &g, uint32_t a, uint32_t b, Sub16 sub)
{
    return hnsw_node_dist(g.base, g.dim, g.metric, g.base + static_cast<int64_t>(b) * g.dim, a, sub);
}

// ---- 1. insert search -----------------------------------------------------------------------------
// pair_base[t] = index of node t's first (node, level) pair counted from node 0 (levels min(level,top)..0
// → pair index + level); the batch's lists are stored relative to pair_base[t0].
// UK: the metric is not Dot, distances are >= +0 and the heaps compare bit patterns (heap_sift_down_uk, vg_heap.hpp)
// levels / pair_base are indexed from node t_base on (the build: 0; vg_hnsw_insert: the first new row)
template <bool UK>
__global__ __launch_bounds__(64) void build_search_kernel(BuildGraph g, int64_t t0, int64_t t_base, uint32_t entry, int cur_top,
                                                          const int32_t *__restrict__ levels,
                                                          const int64_t *__restrict__ pair_base, int ef,
                                                          uint32_t *__restrict__ visited_ws, int64_t vis_words,
                                                          uint32_t *__restrict__ cand_ids,
                                                          float *__restrict__ cand_d, int32_t *__restrict__ cand_n)
{
    extern __shared__ __attribute__((aligned(8))) unsigned char smem[];
    float *nb_pair = reinterpret_cast<float *>(smem);
    float *nb_bnd = nb_pair + 64;
    HItem *cand = reinterpret_cast<HItem *>(nb_bnd + 64);
    HItem *res = cand + 2 * ef;
    const int lane = threadIdx.x;
    const int64_t t = t0 + blockIdx.x;
    F32Scorer sc;
    sc.base = g.base;
    sc.qv = g.base + t * g.dim;
    sc.dim = g.dim;
    sc.metric = g.metric;
    sc.sub = Sub16::make(lane);
    uint32_t *vis = visited_ws + static_cast<int64_t>(blockIdx.x) * vis_words;
    const int lt = levels[t - t_base];
    const int64_t pair0 = pair_base[t - t_base] - pair_base[t0 - t_base];

    uint32_t cur = entry;
    float cur_d = sc.one(cur);
    for (int level = cur_top; level > lt; level--) {  // hnsw.go:918-934
        auto row_of = [&](uint32_t node) -> const uint32_t * { return bg_ids(g, bg_row(g, node, level)); };
        greedy_layer(sc, lane, row_of, g.m, nb_pair, nb_bnd, cur, cur_d);
    }
    const int first = lt < cur_top ? lt : cur_top;
    LayerStats st;
    for (int level = first; level >= 0; level--) {  // hnsw.go:940-957
        if (level != first) {  // initializeSearch: Visited.Reset()
            for (int64_t w = lane; w < vis_words; w += 64) vis[w] = 0;
            __threadfence();
            __syncthreads();
        }
        const int deg = level == 0 ? g.m0 : g.m;
        auto row_of = [&](uint32_t node) -> const uint32_t * { return bg_ids(g, bg_row(g, node, level)); };
        int res_len = 0;
        search_layer<UK>(sc, g.metric == kMetricL2, lane, row_of, deg, cur, cur_d, ef, cand, res, nb_pair, nb_bnd, vis,
                         res_len, st);
        // candidates.MinItem() (queue.go:46-57): the first minimum in heap-array order
        uint64_t best = kKeyMax;
        for (int i = lane; i < res_len; i += 64) {
            const uint64_t key = (static_cast<uint64_t>(f32_ordered(res[i].dist)) << 32) | static_cast<uint32_t>(i);
            best = key < best ? key : best;
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const uint32_t lo = __shfl_xor(static_cast<uint32_t>(best), s);
            const uint32_t hi = __shfl_xor(static_cast<uint32_t>(best >> 32), s);
            const uint64_t o = (static_cast<uint64_t>(hi) << 32) | lo;
            best = o < best ? o : best;
        }
        const HItem bi = res[static_cast<uint32_t>(best)];
        cur = bi.node;
        cur_d = bi.dist;
        // extractSortedCandidates (hnsw.go:1026-1046) / selectNeighborsSimple: pop everything, nearest first
        const int64_t p = pair0 + level;
        const int nres = res_len;
        bool sorted = false;
        if constexpr (UK) {  // no two results tie: the pops' order is the ascending order (vg_hnsw_layer.hpp)
            uint64_t *keys = reinterpret_cast<uint64_t *>(cand);
            sorted = results_sorted_lds(res, nres, keys, nres, lane);
            if (sorted) {
                for (int i = lane; i < nres; i += 64) {
                    cand_ids[p * ef + i] = static_cast<uint32_t>(keys[i]);
                    cand_d[p * ef + i] = __uint_as_float(static_cast<uint32_t>(keys[i] >> 32));
                }
            }
        }
        for (int i = nres - 1; i >= 0 && !sorted; i--) {
            const HItem it = heap_pop<true, UK>(res, res_len);
            if (lane == 0) {
                cand_ids[p * ef + i] = it.node;
                cand_d[p * ef + i] = it.dist;
            }
        }
        if (lane == 0) cand_n[p] = nres;
        __syncthreads();
    }
}

// ---- 2. the new node's own neighbours ----------------------------------------------------------------
// pair_node / pair_level: the (node, level) of every pair of the batch
struct SelShared {
    float dm[64][65];     // pair distances between the members of the final list
    float dtmp[64];       // distances of the candidate under test to the selected ones
    uint32_t fid[64];     // final list: node ids
    float fd[64];         //             their distance to the new node
    int fsel[64];         //             1 = chosen by the heuristic, 0 = filled up
    int flag, nsel, nfinal;
};

// pair_first: index of the batch's first pair among the call's pairs (vg_hnsw_insert's state rows of the new rows)
__global__ __launch_bounds__(kSelThreads) void build_select_kernel(BuildGraph g, int64_t pair_first,
                                                                   const uint32_t *__restrict__ pair_node,
                                                                   const int32_t *__restrict__ pair_level, int ef,
                                                                   const uint32_t *__restrict__ cand_ids,
                                                                   const float *__restrict__ cand_d,
                                                                   const int32_t *__restrict__ cand_n, int rec_stride,
                                                                   uint32_t *__restrict__ rec_row,
                                                                   uint32_t *__restrict__ rec_t, float *__restrict__ rec_d)
{
    __shared__ SelShared sh;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, grp = tid >> 4;
    const Sub16 sub = Sub16::make(tid);
    const uint32_t t = pair_node[p];
    const int level = pair_level[p];
    const int64_t row = bg_row(g, t, level);
    uint32_t *const rid = bg_ids(g, row);
    const int64_t srow = g.smap ? pair_first + p : row;
    const int64_t off = bg_soff(g, row, srow);
    const int m = bg_deg(g, row);
    const int nc = cand_n[p];
    const uint32_t *cid = cand_ids + p * ef;
    const float *cdist = cand_d + p * ef;

    if (nc <= m) {  // selectNeighborsSimple (hnsw.go:993-1009): everything, nearest first
        for (int i = tid; i < nc; i += kSelThreads) {
            sh.fid[i] = cid[i];
            sh.fd[i] = cdist[i];
            sh.fsel[i] = 0;
        }
        if (tid == 0) {
            sh.nsel = 0;
            sh.nfinal = nc;
        }
        __syncthreads();
    } else {
        if (tid == 0) sh.nsel = 0;
        __syncthreads();
        for (int i = 0; i < nc; i++) {  // applyHeuristic (hnsw.go:1048-1085)
            const int nk = sh.nsel;
            if (nk >= m) break;
            const uint32_t id = cid[i];
            const float cd = cdist[i];
            if (tid == 0) sh.flag = 0;
            __syncthreads();
            for (int s0 = 0; s0 < nk; s0 += kSelThreads / 16) {
                const int s = s0 + grp;
                if (s < nk) {
                    const float d = bg_pair(g, id, sh.fid[s], sub);
                    if ((tid & 15) == 0) {
                        sh.dtmp[s] = d;
                        if (d < cd) sh.flag = 1;
                    }
                }
            }
            __syncthreads();
            if (!sh.flag) {
                for (int s = tid; s < nk; s += kSelThreads) {
                    sh.dm[nk][s] = sh.dtmp[s];
                    sh.dm[s][nk] = sh.dtmp[s];
                }
                if (tid == 0) {
                    sh.fid[nk] = id;
                    sh.fd[nk] = cd;
                    sh.fsel[nk] = 1;
                    sh.nsel = nk + 1;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {  // fillUpNeighbors (hnsw.go:1087-1106)
            int nk = sh.nsel;
            const int nsel = nk;
            for (int i = 0; i < nc && nk < m; i++) {
                bool found = false;
                for (int s = 0; s < nsel; s++) found |= sh.fid[s] == cid[i];
                if (!found) {
                    sh.fid[nk] = cid[i];
                    sh.fd[nk] = cdist[i];
                    sh.fsel[nk] = 0;
                    nk++;
                }
            }
            sh.nfinal = nk;
        }
        __syncthreads();
    }
    // pair distances the heuristic did not need: every pair with a filled-up member
    const int nf = sh.nfinal, nsel = sh.nsel;
    const int nfill = nf - nsel;
    for (int e0 = 0; e0 < nfill * nf; e0 += kSelThreads / 16) {
        const int e = e0 + grp;
        if (e < nfill * nf) {
            const int a = nsel + e / nf, b = e % nf;
            if (b < a) {  // b selected, or an earlier fill-up
                const float d = bg_pair(g, sh.fid[a], sh.fid[b], sub);
                if ((tid & 15) == 0) {
                    sh.dm[a][b] = d;
                    sh.dm[b][a] = d;
                }
            }
        }
    }
    __syncthreads();
    // the row: setConnections (hnsw.go:445-453), plus the bit matrix, plus one back-link record per member
    for (int i = tid; i < m; i += kSelThreads) {
        uint64_t bits = 0;
        if (i < nf) {
            const float di = sh.fd[i];
            for (int j = 0; j < nf; j++)
                if (j != i && sh.dm[i][j] < di) bits |= 1ull << j;
        }
        rid[i] = i < nf ? sh.fid[i] : VG_INVALID_ID;
        g.dist[off + i] = i < nf ? sh.fd[i] : 0.0f;
        g.bits[off + i] = bits;
        if (i < rec_stride) {
            const uint32_t trow = i < nf ? static_cast<uint32_t>(bg_row(g, sh.fid[i], level)) : VG_INVALID_ID;
            if (g.row_node && i < nf) g.row_node[trow] = sh.fid[i];  // (every writer of a row writes the same node)
            rec_row[p * rec_stride + i] = trow;
            rec_t[p * rec_stride + i] = t;
            rec_d[p * rec_stride + i] = i < nf ? sh.fd[i] : 0.0f;
        }
    }
    for (int i = m + tid; i < rec_stride; i += kSelThreads) rec_row[p * rec_stride + i] = VG_INVALID_ID;
    if (tid == 0) {
        g.cnt[srow] = nf;
        g.good[srow] = nf == m && nsel == m ? 1 : 0;
        if (g.smap) {
            g.smap[row] = static_cast<int32_t>(srow);
            g.srow_row[srow] = static_cast<uint32_t>(row);
        }
    }
}

// ---- 3. back links ---------------------------------------------------------------------------------
struct LinkTotals {  // over the whole build (VG_BUILD_DEBUG prints them)
    unsigned long long records, skipped, appended, pruned, good_rows_seen, longest_chain;
    unsigned long long skipped_stable;  // of `skipped`: on a row with tied members, by `stable`
    // rows with >= 1000 records in a batch (hubs), 100 MHz ticks: where one workgroup's time goes
    unsigned long long hub_rows, hub_records, hub_applied, hub_sort, hub_scan, hub_gather, hub_replay, hub_total, hub_ties, max_wg;
};

__global__ void build_fill_kernel(const uint32_t *__restrict__ rec_row, const uint32_t *__restrict__ rec_t,
                                  const float *__restrict__ rec_d, int64_t nrec, const uint32_t *__restrict__ roff,
                                  int32_t *__restrict__ rfill, uint32_t *__restrict__ srt_t, float *__restrict__ srt_d)
{
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= nrec) return;
    const uint32_t row = rec_row[r];
    if (row == VG_INVALID_ID) return;
    const uint32_t pos = roff[row] + static_cast<uint32_t>(atomicAdd(&rfill[row], 1));
    srt_t[pos] = rec_t[r];
    srt_d[pos] = rec_d[r];
}

struct LinkShared {
    HItem heap[65];
    float pd[64];
    float cd[65];          // candidate distances (slot 0..deg-1, then the new node)
    uint64_t cbits[65];    // bits over the old slots
    uint32_t ctbit[65];    // bit against the new node
    uint32_t cid[65];
    int seq[65];           // candidates in the order extractSortedCandidates would give (nearest first)
    int newpos[65];        // their slot after the prune, -1 = dropped
    uint32_t mid[64];      // the row's member ids, for the scoring waves
    uint32_t t;            // the record being applied
    int action;            // 0 = nothing to score for this record, 1 = score the new node against the members
    int cnt;
};

constexpr int kLinkWaves = 4;
constexpr int kLinkThreads = kLinkWaves * 64;

// LDS hand-over inside ONE wave (the bookkeeping wave below): its LDS instructions execute in order, so all it takes
// is that the compiler does not move them across this point
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One workgroup of four waves per target row: the row's records in ascending id of the new node (the order a
// sequential pass over the batch applies them), each one = addConnection (hnsw.go:455-499).  Wave 0 keeps the row
// (lane i = slot i: id, cached distance, bit row) and does the bookkeeping; for a record that needs them, the 64
// distances between the new node and the row's members are scored by all four waves at once (16 members each, 4
// rows in flight per wave).  A row's records are a serial chain — a hub row (near to very many nodes, as
// high-dimensional data has them) can receive thousands per batch — so what counts is the latency of one link.
__global__ __launch_bounds__(kLinkThreads) void build_link_kernel(BuildGraph g, const uint32_t *__restrict__ work,
                                                                  const GroupCounters *__restrict__ ctr,
                                                                  int32_t *__restrict__ rcnt, int32_t *__restrict__ rfill,
                                                                  const uint32_t *__restrict__ roff,
                                                                  const uint32_t *__restrict__ srt_t,
                                                                  const float *__restrict__ srt_d,
                                                                  uint32_t *__restrict__ ord, float *__restrict__ ord_d,
                                                                  LinkTotals *__restrict__ totals)
{
    __shared__ LinkShared sh;
    if (blockIdx.x >= ctr->nwork) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Sub16 sub = Sub16::make(lane);
    const int64_t row = work[blockIdx.x];
    uint32_t *const rid = bg_ids(g, row);
    const int64_t srow = g.smap ? g.smap[row] : row;
    const int64_t off = bg_soff(g, row, srow);
    const int deg = bg_deg(g, row);
    const int nadd = rcnt[row];
    const uint32_t *at = srt_t + roff[row];
    const float *ad = srt_d + roff[row];
    const unsigned long long tk_all = totals ? wall_clock64() : 0;
    const bool timed = totals != nullptr && nadd >= 1000;
    unsigned long long tk_sort = 0, tk_scan = 0, tk_gather = 0, tk_replay = 0;
    const unsigned long long tk_begin = timed ? wall_clock64() : 0;
    uint32_t *st = ord + roff[row];   // the row's records in ascending t (distinct per row): new node ...
    float *sd = ord_d + roff[row];    // ... and its distance to the row's node
    for (int i = tid; i < nadd; i += kLinkThreads) {  // rank sort by the whole workgroup, once
        const uint32_t ti = at[i];
        int rank = 0;
        for (int j = 0; j < nadd; j++) rank += at[j] < ti ? 1 : 0;
        st[rank] = ti;
        sd[rank] = ad[i];
    }
    __threadfence_block();
    __syncthreads();
    if (timed) tk_sort = wall_clock64() - tk_begin;

    // row state: wave 0 only
    int cnt = 0;
    uint32_t id = VG_INVALID_ID;
    float dist = 0.0f;
    uint64_t bits = 0;
    bool good = false, ties = false;
    bool stable = false;  // a good row WITH ties that a far record was seen to leave exactly as it is (see below)
    unsigned int n_skip = 0, n_skip_stable = 0, n_app = 0, n_prune = 0, n_tie = 0;
    auto row_has_ties = [&]() {
        const float nxt = __shfl_down(dist, 1);
        return __ballot(lane + 1 < cnt && dist == nxt) != 0;
    };
    if (wave == 0) {
        cnt = g.cnt[srow];
        id = lane < deg ? rid[lane] : VG_INVALID_ID;
        dist = lane < deg ? g.dist[off + lane] : 0.0f;
        bits = lane < deg ? g.bits[off + lane] : 0;
        // The cheap way out.  `good` = the row is full and applyHeuristic CHOSE every member (nothing was filled up),
        // so the row is in ascending distance order.  A new node farther than the farthest member then sorts last, the
        // heuristic re-chooses the 64 members, stops (len(result) >= m, hnsw.go:1054) and never looks at the newcomer:
        // the row is left exactly as it is — unless two members are equally far, in which case the reference's heap
        // may hand them back in another order, so a row with ties takes the long way ONCE: a newcomer farther than
        // every member compares the same way against everything whatever its distance, so if one such record leaves the
        // row exactly as it was (every member re-chosen, in the same slots), every later one will too, until the row
        // changes (`stable`).  Hub rows — thousands of back links per batch, and two bit-equal cached distances among
        // their 64 almost always — would otherwise replay the heap for every record.  75 % of the back links of the
        // 1M x 768 build end here.
        good = g.good[srow] != 0;
        ties = row_has_ties();
        sh.mid[lane] = id;
    }

    // Wave 0 walks the records 64 at a time (one coalesced load per chunk, lane i = record chunk*64 + i) and tests
    // the cheap way out for a whole chunk at once: the row's state only changes when a record is actually applied,
    // so everything up to the first record that needs work is skipped without a barrier or a memory access.  The
    // other waves only see the records that need their 64 distances.
    int a = 0, chunk = -1;
    uint32_t ct = 0;
    float cdist = 0.0f;
    for (;;) {
        uint32_t t = 0;
        float dt = 0.0f;
        const unsigned long long tk0 = timed ? wall_clock64() : 0;
        if (wave == 0) {
            int action = 2;  // 2 = no record left
            while (a < nadd) {
                if ((a >> 6) != chunk) {
                    chunk = a >> 6;
                    const int i = chunk * 64 + lane;
                    ct = i < nadd ? st[i] : 0u;
                    cdist = i < nadd ? sd[i] : 0.0f;
                }
                const int i = chunk * 64 + lane;
                const bool pending = i >= a && i < nadd;
                const bool far = cnt == deg && good && (!ties || stable) && cdist > __shfl(dist, deg - 1);
                const uint64_t work = __ballot(pending && !far);  // records of this chunk that need a closer look
                const int rest = nadd - chunk * 64 < 64 ? nadd - chunk * 64 : 64;  // records in this chunk
                const int f = work ? __builtin_ctzll(work) : rest;                  // lane of the first of them
                n_skip += static_cast<unsigned int>(f - (a & 63));
                if (ties && stable) n_skip_stable += static_cast<unsigned int>(f - (a & 63));
                a = chunk * 64 + f;
                if (f == rest) continue;  // the chunk is done: next chunk (or the end)
                t = __shfl(ct, f);
                dt = __shfl(cdist, f);
                a++;
                if (__ballot(lane < cnt && id == t)) continue;  // already connected (hnsw.go:477-486)
                action = 1;
                break;
            }
            if (lane == 0) {
                sh.t = t;
                sh.action = action;
                sh.cnt = cnt;
            }
        }
        __syncthreads();
        const unsigned long long tk1 = timed ? wall_clock64() : 0;
        tk_scan += tk1 - tk0;
        if (sh.action == 2) break;
        {   // distances between the new node and the row's members: wave w scores members 16w .. 16w+15
            const uint32_t tt = sh.t;
            const int c = sh.cnt;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = wave * 16 + r * 4 + (lane >> 4);
                if (j < c) {
                    const float d = bg_pair(g, sh.mid[j], tt, sub);
                    if ((lane & 15) == 0) sh.pd[j] = d;
                }
            }
        }
        __syncthreads();
        const unsigned long long tk2 = timed ? wall_clock64() : 0;
        tk_gather += tk2 - tk1;
        if (wave == 0) {
            const float pd = lane < cnt ? sh.pd[lane] : 0.0f;
            const uint64_t tbits = __ballot(lane < cnt && pd < dt);       // row of the new node
            const uint32_t colbit = (lane < cnt && pd < dist) ? 1u : 0u;  // bit (member, new node)
            if (cnt < deg) {  // addConnectionSimple (hnsw.go:501-518)
                if (lane < cnt) bits |= static_cast<uint64_t>(colbit) << cnt;
                if (lane == cnt) {
                    id = t;
                    dist = dt;
                    bits = tbits;
                }
                cnt++;
                n_app++;
                stable = false;
                good = false;  // appended, not chosen
                ties = row_has_ties();
            } else {
                // addConnectionPrune (hnsw.go:520-555): members in list order, then the new node, through the max-heap
                // and back out nearest first.  Distinct distances: the order is the sort by distance.  Equal
                // distances: whatever the heap does, so the heap is replayed.
                n_prune++;
                const bool was_far = good && dt > __shfl(dist, deg - 1);  // farther than every member of a fully chosen row
                const int nc = deg + 1;
                if (lane < deg) {
                    sh.cd[lane] = dist;
                    sh.cbits[lane] = bits;
                    sh.ctbit[lane] = colbit;
                    sh.cid[lane] = id;
                }
                if (lane == 0) {
                    sh.cd[deg] = dt;
                    sh.cbits[deg] = tbits;
                    sh.ctbit[deg] = 0;
                    sh.cid[deg] = t;
                }
                wave_sync();
                int rank = 0;
                bool tie = false;
                if (lane < deg) {
                    for (int j = 0; j < nc; j++) {
                        const float dj = sh.cd[j];
                        rank += dj < dist ? 1 : 0;
                        tie |= (j != lane) && dj == dist;
                    }
                }
                int rank_t = 0;
                for (int j = 0; j < deg; j++) rank_t += sh.cd[j] < dt ? 1 : 0;
                if (__ballot(tie)) {
                    n_tie++;
                    int hl = 0;
                    for (int j = 0; j < nc; j++) heap_push<true>(sh.heap, hl, HItem{static_cast<uint32_t>(j), sh.cd[j]});
                    for (int j = nc - 1; j >= 0; j--) {
                        const HItem it = heap_pop<true>(sh.heap, hl);
                        if (lane == 0) sh.seq[j] = static_cast<int>(it.node);
                    }
                } else {
                    if (lane < deg) sh.seq[rank] = lane;
                    if (lane == 0) sh.seq[rank_t] = deg;
                }
                wave_sync();
                // applyHeuristic + fillUpNeighbors over the bit rows.  The greedy pass is sequential by nature; what
                // it reads is brought into registers first — lane p: the candidate at sorted position p, its bit row and
                // its bit against the new node (position 64, the last of 65, is kept as scalars) — so that a step is a
                // few readlanes instead of a chain of dependent LDS reads (this loop was half of a back link's time).
                const int my_ci = sh.seq[lane < nc ? lane : 0];
                const uint64_t my_cb = sh.cbits[my_ci];
                const uint32_t my_ctb = sh.ctbit[my_ci];
                const int last_ci = sh.seq[nc - 1];  // only meaningful when nc == 65
                const uint64_t last_cb = sh.cbits[last_ci];
                const uint32_t last_ctb = sh.ctbit[last_ci];
                int my_newpos = -1;  // lane j < deg: new slot of member j
                int newpos_t = -1;   // new slot of the new node
                uint64_t selmask = 0;
                bool sel_t = false;
                int nsel = 0;
                for (int p = 0; p < nc && nsel < deg; p++) {
                    int ci;
                    uint64_t cb;
                    uint32_t ctb;
                    if (p < 64) {
                        ci = __builtin_amdgcn_readlane(my_ci, p);
                        cb = readlane_u64(my_cb, p);
                        ctb = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(my_ctb), p));
                    } else {
                        ci = last_ci;
                        cb = last_cb;
                        ctb = last_ctb;
                    }
                    const bool bad = (cb & selmask) != 0 || (ctb != 0 && sel_t);
                    if (!bad) {
                        if (ci == deg) {
                            sel_t = true;
                            newpos_t = nsel;
                        } else {
                            selmask |= 1ull << ci;
                            if (lane == ci) my_newpos = nsel;
                        }
                        nsel++;
                    }
                }
                const int nchosen = nsel;
                for (int p = 0; p < nc && nsel < deg; p++) {
                    const int ci = p < 64 ? __builtin_amdgcn_readlane(my_ci, p) : last_ci;
                    const bool chosen = ci == deg ? sel_t : ((selmask >> ci) & 1) != 0;
                    if (!chosen) {
                        if (ci == deg)
                            newpos_t = nsel;
                        else if (lane == ci)
                            my_newpos = nsel;
                        nsel++;
                    }
                }
                // the row in its new order (slot -> candidate through an LDS scatter); the columns of the bit matrix
                // move with their members
                sh.newpos[lane] = -1;  // reused as slot -> candidate
                wave_sync();
                if (lane < deg && my_newpos >= 0) sh.newpos[my_newpos] = lane;
                if (lane == 0 && newpos_t >= 0) sh.newpos[newpos_t] = deg;
                wave_sync();
                const int src = sh.newpos[lane];
                uint64_t nb = 0;
                if (src >= 0) {
                    const uint64_t ob = sh.cbits[src];
                    for (int j = 0; j < deg; j++) {
                        const int np = __builtin_amdgcn_readlane(my_newpos, j);
                        if (np >= 0) nb |= ((ob >> j) & 1ull) << np;
                    }
                    if (newpos_t >= 0) nb |= static_cast<uint64_t>(sh.ctbit[src]) << newpos_t;
                    id = sh.cid[src];
                    dist = sh.cd[src];
                } else {
                    id = VG_INVALID_ID;
                    dist = 0.0f;
                }
                const bool unchanged = newpos_t < 0 && __ballot(lane < deg && src != lane) == 0;
                bits = nb;
                cnt = nsel;
                good = nchosen == deg;
                ties = row_has_ties();
                if (!unchanged)
                    stable = false;
                else if (was_far && good)
                    stable = true;
            }
            wave_sync();
            sh.mid[lane] = id;
        }
        __syncthreads();
        if (timed) tk_replay += wall_clock64() - tk2;
    }
    if (wave == 0) {
        if (lane < deg) {
            rid[lane] = lane < cnt ? id : VG_INVALID_ID;
            g.dist[off + lane] = lane < cnt ? dist : 0.0f;
            g.bits[off + lane] = lane < cnt ? bits : 0;
        }
        if (lane == 0) {
            if (totals) {
                atomicAdd(&totals->records, static_cast<unsigned long long>(nadd));
                atomicAdd(&totals->skipped, static_cast<unsigned long long>(n_skip));
                atomicAdd(&totals->skipped_stable, static_cast<unsigned long long>(n_skip_stable));
                atomicAdd(&totals->appended, static_cast<unsigned long long>(n_app));
                atomicAdd(&totals->pruned, static_cast<unsigned long long>(n_prune));
                atomicAdd(&totals->good_rows_seen, static_cast<unsigned long long>(g.good[srow] ? 1 : 0));
                atomicMax(&totals->longest_chain, static_cast<unsigned long long>(nadd));
                if (timed) {
                    atomicAdd(&totals->hub_rows, 1ull);
                    atomicAdd(&totals->hub_records, static_cast<unsigned long long>(nadd));
                    atomicAdd(&totals->hub_applied, static_cast<unsigned long long>(n_app + n_prune));
                    atomicAdd(&totals->hub_sort, tk_sort);
                    atomicAdd(&totals->hub_scan, tk_scan);
                    atomicAdd(&totals->hub_gather, tk_gather);
                    atomicAdd(&totals->hub_replay, tk_replay);
                    atomicAdd(&totals->hub_total, wall_clock64() - tk_begin);
                    atomicAdd(&totals->hub_ties, static_cast<unsigned long long>(n_tie));
                }
                {
                    const unsigned long long tk = wall_clock64() - tk_all;
                    atomicMax(&totals->max_wg, (tk << 40) | (static_cast<unsigned long long>(nadd & 0xFFFF) << 24) |
                                                   (static_cast<unsigned long long>(n_prune & 0xFFFF) << 8) | (n_tie > 255 ? 255 : n_tie));
                }
            }
            g.cnt[srow] = cnt;
            g.good[srow] = good ? 1 : 0;
            rcnt[row] = 0;
            rfill[row] = 0;
        }
    }
}

__global__ void fill_u32_kernel(uint32_t *p, int64_t n, uint32_t v)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- vg_hnsw_insert: build state of a row that existed before the call -------------------------------
// One workgroup per row of the batch's work list that has no state row yet (one the build would have kept from
// the insert that made it): its member ids come from the graph; dist[i] = the distance the row cached for member i;
// bits[i] bit j = d(member i, member j) < dist[i], the pair distances by the reference's kernel in its summation order
// (what the build compared: symmetric bit for bit).  dist comes from the cached distances the index keeps for a graph
// it built (d_hnsw_*_cdist) — they cannot be recomputed: the insert search caches the bounded kernel's sum once its
// result heap is full, another summation order — else from the uploaded layer-0 edge distances, else it is
// d(row's node, member i) by the pair kernel.  good = 0: the first record that reaches the full row takes
// addConnectionPrune's long path, which gives what the shortcut gives.  Runs after the count kernel (the work
// list) and before the link kernel; the rows are distinct within a batch.
struct DeriveShared {
    float dm[64][65];
    float md[64];
    uint32_t mid[64];
    int64_t srow;
    int cnt, fresh;
};

__global__ __launch_bounds__(kSelThreads) void build_derive_kernel(BuildGraph g, const uint32_t *__restrict__ work,
                                                                   const GroupCounters *__restrict__ ctr,
                                                                   unsigned int *__restrict__ s_next, int64_t s_first,
                                                                   const float *__restrict__ l0_dist, int64_t dist_rows,
                                                                   const float *__restrict__ cd0, const float *__restrict__ cdu,
                                                                   unsigned int *__restrict__ derived)
{
    __shared__ DeriveShared sh;
    if (blockIdx.x >= ctr->nwork) return;
    const int tid = threadIdx.x, grp = tid >> 4;
    const Sub16 sub = Sub16::make(tid);
    const int64_t row = work[blockIdx.x];
    const int deg = bg_deg(g, row);
    const uint32_t *rid = bg_ids(g, row);
    if (tid == 0) {
        int64_t s = g.smap[row];
        sh.fresh = s < 0 ? 1 : 0;
        if (s < 0) {
            s = s_first + atomicAdd(s_next, 1u);
            g.smap[row] = static_cast<int32_t>(s);
            g.srow_row[s] = static_cast<uint32_t>(row);
            atomicAdd(derived, 1u);
        }
        sh.srow = s;
        int c = 0;
        while (c < deg && rid[c] != VG_INVALID_ID) c++;
        sh.cnt = c;
    }
    __syncthreads();
    if (!sh.fresh) return;
    const int cnt = sh.cnt;
    const uint32_t node = g.row_node[row];
    if (tid < cnt) sh.mid[tid] = rid[tid];
    __syncthreads();
    for (int i0 = 0; i0 < cnt; i0 += kSelThreads / 16) {
        const int i = i0 + grp;
        if (i < cnt) {
            float d;
            if (cd0)
                d = row < g.n ? cd0[row * g.m0 + i] : cdu[(row - g.n) * g.m + i];
            else if (l0_dist && row < dist_rows)
                d = l0_dist[row * g.m0 + i];
            else
                d = bg_pair(g, sh.mid[i], node, sub);
            if ((tid & 15) == 0) sh.md[i] = d;
        }
    }
    const int npair = cnt * (cnt - 1) / 2;
    for (int e0 = 0; e0 < npair; e0 += kSelThreads / 16) {
        const int e = e0 + grp;
        if (e < npair) {  // e = a (a - 1) / 2 + b, b < a
            int a = static_cast<int>((1.0f + sqrtf(1.0f + 8.0f * static_cast<float>(e))) * 0.5f);
            while (a * (a - 1) / 2 > e) a--;
            while ((a + 1) * a / 2 <= e) a++;
            const int b = e - a * (a - 1) / 2;
            const float d = bg_pair(g, sh.mid[a], sh.mid[b], sub);
            if ((tid & 15) == 0) {
                sh.dm[a][b] = d;
                sh.dm[b][a] = d;
            }
        }
    }
    __syncthreads();
    const int64_t srow = sh.srow;
    const int64_t off = srow * kStateStride;
    for (int i = tid; i < deg; i += kSelThreads) {
        uint64_t bits = 0;
        if (i < cnt) {
            const float di = sh.md[i];
            for (int j = 0; j < cnt; j++)
                if (j != i && sh.dm[i][j] < di) bits |= 1ull << j;
        }
        g.dist[off + i] = i < cnt ? sh.md[i] : 0.0f;
        g.bits[off + i] = bits;
    }
    if (tid == 0) {
        g.cnt[srow] = cnt;
        g.good[srow] = 0;
    }
}

// after the batches: every state row's cached distances back into the index's (l0 / upper) arrays
__global__ void state_writeback_kernel(BuildGraph g, const unsigned int *__restrict__ s_next, int64_t npairs,
                                       float *__restrict__ cd0, float *__restrict__ cdu)
{
    const int64_t s = blockIdx.x;
    if (s >= npairs + static_cast<int64_t>(*s_next)) return;
    const int64_t row = g.srow_row[s];
    const int deg = bg_deg(g, row);
    float *dst = row < g.n ? cd0 + row * g.m0 : cdu + (row - g.n) * g.m;
    for (int i = threadIdx.x; i < deg; i += blockDim.x) dst[i] = g.dist[s * kStateStride + i];
}

// the upper slot table of n_new nodes from the old one (n_old nodes, L_old levels) and the new nodes' slots
// (fresh[l * count + (i - n_old)])
__global__ void slot_relayout_kernel(const uint32_t *__restrict__ old, int64_t n_old, int l_old,
                                     const uint32_t *__restrict__ fresh, int64_t n_new, int l_new,
                                     uint32_t *__restrict__ out)
{
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= static_cast<int64_t>(l_new) * n_new) return;
    const int l = static_cast<int>(e / n_new);
    const int64_t i = e - static_cast<int64_t>(l) * n_new;
    uint32_t v;
    if (i >= n_old)
        v = fresh[static_cast<int64_t>(l) * (n_new - n_old) + (i - n_old)];
    else
        v = l < l_old ? old[static_cast<int64_t>(l) * n_old + i] : VG_INVALID_ID;
    out[e] = v;
}

// tombstone bits from `from` to the end of the byte that holds bit to - 1 cleared (little-endian bit order, as
// the searches read them): the new rows are live
__global__ void clear_bits_kernel(uint8_t *__restrict__ bm, int64_t from, int64_t to)
{
    const int64_t byte = from / 8 + static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (byte * 8 >= to) return;
    uint8_t keep = 0;
    for (int b = 0; b < 8; b++)
        if (byte * 8 + b < from) keep |= static_cast<uint8_t>(1u << b);
    bm[byte] &= keep;
}

// Everything the batches of one call read or write besides the graph and the plan (device pointers): carve_run
struct BuildRun {
    int ef = 0;
    int32_t *levels = nullptr;  // the plan's levels / pair_base / pair_node / pair_level
    int64_t *pair_base = nullptr;
    uint32_t *pair_node = nullptr;
    int32_t *pair_level = nullptr;
    uint32_t *vis = nullptr, *cand_ids = nullptr;
    float *cand_d = nullptr;
    int32_t *cand_n = nullptr;
    uint32_t *rec_row = nullptr, *rec_t = nullptr, *srt_t = nullptr, *ord = nullptr, *work = nullptr, *roff = nullptr;
    float *rec_d = nullptr, *srt_d = nullptr, *ordd = nullptr;
    int32_t *rcnt = nullptr, *rfill = nullptr;  // zero on entry; the link kernel leaves them zero
    GroupCounters *ctr = nullptr;
    LinkTotals *totals = nullptr;  // VG_BUILD_DEBUG only
    // vg_hnsw_insert (g.smap set): state rows of the rows existing before the call come from s_first + *s_next
    unsigned int *s_next = nullptr, *derived = nullptr;
    int64_t s_first = 0, n_state = 0;
    const float *l0_dist = nullptr;  // uploaded layer-0 edge distances of rows < dist_rows, or null
    int64_t dist_rows = 0;
    const float *cd0 = nullptr, *cdu = nullptr;  // the index's cached distances (layer 0, upper), or null
};

// Every per-call scratch piece of run_batches with its size: the plan's device copy, the batches' buffers (sized by
// the call's largest batch) and, for vg_hnsw_insert, the state rows.  base null: returns the bytes the call needs;
// else points r (and, insert, g's state) into them.
static size_t carve_run(char *base, const HnswBuildPlan &p, int m0, bool insert, BuildRun &r, BuildGraph &g)
{
    Carve c{base};
    const int64_t npairs = p.pair_base[p.count], max_rec = p.max_pairs * m0;
    c.take(r.levels, p.count);
    c.take(r.pair_base, p.count + 1);
    c.take(r.pair_node, npairs);
    c.take(r.pair_level, npairs);
    c.take(r.vis, p.max_b * ((p.n_old + p.count + 31) / 32));  // one visited bitmap per node of a batch
    c.take(r.cand_ids, p.max_pairs * r.ef);
    c.take(r.cand_d, p.max_pairs * r.ef);
    c.take(r.cand_n, p.max_pairs);
    for (uint32_t **q : {&r.rec_row, &r.rec_t, &r.srt_t, &r.ord}) c.take(*q, max_rec);
    for (float **q : {&r.rec_d, &r.srt_d, &r.ordd}) c.take(*q, max_rec);
    c.take(r.work, std::min(max_rec, p.total_rows));
    c.take(r.roff, p.total_rows);
    c.take(r.rcnt, p.total_rows);
    c.take(r.rfill, p.total_rows);
    c.take(r.ctr, 1);
    c.take(r.totals, 1);
    if (!hook(kHookBuildDebug)) r.totals = nullptr;
    if (insert) {
        // state rows: one per new (node, level) pair, then one per derived row.  A row is derived at most once per call
        // and only when a record targets it: at most one per record, at most one per row.  (Derived rows are the graph's
        // older rows and the rows a new node gets above the top level of its batch, which no pair makes.)
        r.s_first = npairs;
        r.n_state = npairs + std::min(p.total_rows, npairs * m0);
        c.take(g.smap, p.total_rows);
        c.take(g.row_node, p.total_rows);
        c.take(g.srow_row, r.n_state);
        c.take(g.dist, r.n_state * kStateStride);
        c.take(g.bits, r.n_state * kStateStride);
        c.take(g.cnt, r.n_state);
        c.take(g.good, r.n_state);
        c.take(r.s_next, 2);
        r.derived = r.s_next + 1;
    }
    return c.off;
}

// VG_BUILD_DEBUG, after a batch: its wall time and its longest per-row chain (a running maximum on the device: reset
// here), every 16th batch printed.  tools/hnsw_build_debug.py reads the lines.
struct BatchDebug {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    unsigned long long max_chain = 0;
};
static int32_t debug_batch(const char *fn, hipStream_t st, LinkTotals *totals, size_t bi, size_t nbatches, int64_t size,
                           BatchDebug &dbg)
{
    VG_HIP(hipStreamSynchronize(st));
    const auto now = std::chrono::steady_clock::now();
    LinkTotals t{};
    VG_HIP(hipMemcpy(&t, totals, sizeof(t), hipMemcpyDeviceToHost));
    if (bi % 16 == 0 || bi + 1 == nbatches)
        fprintf(stderr, "%s: batch %zu: %lld nodes, %.2f ms, longest chain %llu; longest link workgroup %.2f ms "
                        "(%llu records, %llu pruned, %llu heap replays)\n", fn, bi, static_cast<long long>(size),
                std::chrono::duration<double, std::milli>(now - dbg.t0).count(), t.longest_chain, (t.max_wg >> 40) / 1e5,
                (t.max_wg >> 24) & 0xFFFF, (t.max_wg >> 8) & 0xFFFF, t.max_wg & 0xFF);
    dbg.t0 = now;
    dbg.max_chain = std::max(dbg.max_chain, t.longest_chain);
    const unsigned long long zero = 0;
    VG_HIP(hipMemcpy(&totals->longest_chain, &zero, sizeof(zero), hipMemcpyHostToDevice));
    VG_HIP(hipMemcpy(&totals->max_wg, &zero, sizeof(zero), hipMemcpyHostToDevice));
    return VG_OK;
}

// The batches, in order: search -> select -> group the back links by target row -> (insert: derive the state of
// target rows that have none) -> link.  vg_hnsw_build and vg_hnsw_insert both run their plan through here; it starts
// with the plan's copy to the device and the zeros the kernels count on, and returns with the stream idle.
static int32_t run_batches(vg_ctx *ctx, hipStream_t st, const BuildGraph &g, const HnswBuildPlan &p, const BuildRun &r,
                           const char *fn)
{
    VG_HIP(hipMemcpyAsync(r.levels, p.levels.data(), p.levels.size() * 4, hipMemcpyHostToDevice, st));
    VG_HIP(hipMemcpyAsync(r.pair_base, p.pair_base.data(), p.pair_base.size() * 8, hipMemcpyHostToDevice, st));
    VG_HIP(hipMemcpyAsync(r.pair_node, p.pair_node.data(), p.pair_node.size() * 4, hipMemcpyHostToDevice, st));
    VG_HIP(hipMemcpyAsync(r.pair_level, p.pair_level.data(), p.pair_level.size() * 4, hipMemcpyHostToDevice, st));
    VG_HIP(hipMemsetAsync(r.rcnt, 0, static_cast<size_t>(p.total_rows) * 4, st));
    VG_HIP(hipMemsetAsync(r.rfill, 0, static_cast<size_t>(p.total_rows) * 4, st));
    if (r.totals) VG_HIP(hipMemsetAsync(r.totals, 0, sizeof(LinkTotals), st));
    if (g.smap) {
        VG_HIP(hipMemsetAsync(g.smap, 0xFF, static_cast<size_t>(p.total_rows) * 4, st));
        VG_HIP(hipMemsetAsync(r.s_next, 0, 8, st));
    }
    const int ef = r.ef, m0 = g.m0;
    const size_t lds = static_cast<size_t>(3 * ef + 4) * sizeof(HItem) + 128 * sizeof(float);
    auto search_kern = g.metric != VG_METRIC_DOT ? build_search_kernel<true> : build_search_kernel<false>;
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(search_kern),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    BatchDebug dbg;
    for (const BuildBatch &bt : p.batches) {
        const int64_t vis_words = (bt.t0 + 31) / 32;  // only nodes below t0 are reachable
        const int64_t nrec = bt.npairs * m0;
        VG_HIP(hipMemsetAsync(r.vis, 0, static_cast<size_t>(bt.size * vis_words) * 4, st));
        {
            ProfScope prof(ctx, "hnsw_build_search", st);
            VG_LAUNCH(search_kern, dim3(static_cast<unsigned>(bt.size)), dim3(64), lds, st, g, bt.t0, p.n_old, bt.entry,
                      bt.cur_top, r.levels, r.pair_base, ef, r.vis, vis_words, r.cand_ids, r.cand_d, r.cand_n);
        }
        const int64_t pb = p.pair_base[bt.t0 - p.n_old];
        {
            ProfScope prof(ctx, "hnsw_build_select", st);
            VG_LAUNCH(build_select_kernel, dim3(static_cast<unsigned>(bt.npairs)), dim3(kSelThreads), 0, st, g, pb,
                      r.pair_node + pb, r.pair_level + pb, ef, r.cand_ids, r.cand_d, r.cand_n, m0,
                      r.rec_row, r.rec_t, r.rec_d);
        }
        const int64_t max_work = std::min(nrec, p.total_rows);
        auto link = [&]() -> int32_t {
            VG_LAUNCH(build_link_kernel, dim3(static_cast<unsigned>(max_work)), dim3(kLinkThreads), 0, st, g, r.work,
                      r.ctr, r.rcnt, r.rfill, r.roff, r.srt_t, r.srt_d, r.ord, r.ordd, r.totals);
            return VG_OK;
        };
        {
            ProfScope prof(ctx, "hnsw_build_link", st);
            VG_TRY(group_count_offsets(r.rec_row, nrec, max_work, r.rcnt, r.work, r.roff, r.ctr, st));
            VG_LAUNCH(build_fill_kernel, dim3(static_cast<unsigned>((nrec + 255) / 256)), dim3(256), 0, st, r.rec_row,
                      r.rec_t, r.rec_d, nrec, r.roff, r.rfill, r.srt_t, r.srt_d);
            if (!g.smap) VG_TRY(link());
        }
        if (g.smap) {
            {
                ProfScope prof(ctx, "hnsw_insert_derive", st);
                VG_LAUNCH(build_derive_kernel, dim3(static_cast<unsigned>(max_work)), dim3(kSelThreads), 0, st, g, r.work,
                          r.ctr, r.s_next, r.s_first, r.l0_dist, r.dist_rows, r.cd0, r.cdu, r.derived);
            }
            ProfScope prof(ctx, "hnsw_build_link", st);
            VG_TRY(link());
        }
        if (r.totals)
            VG_TRY(debug_batch(fn, st, r.totals, static_cast<size_t>(&bt - p.batches.data()), p.batches.size(), bt.size, dbg));
    }
    VG_HIP(hipStreamSynchronize(st));
    if (r.totals) {
        LinkTotals t{};
        VG_HIP(hipMemcpy(&t, r.totals, sizeof(t), hipMemcpyDeviceToHost));
        fprintf(stderr, "%s: back links %llu = %llu skipped (farther than a fully chosen row's last member; %llu of them on a "
                        "settled row with tied members) + %llu appended + "
                        "%llu pruned; target-row visits that found the row fully chosen %llu; longest per-row chain in one batch %llu\n",
                fn, t.records, t.skipped, t.skipped_stable, t.appended, t.pruned, t.good_rows_seen,
                std::max(dbg.max_chain, t.longest_chain));
        fprintf(stderr, "%s: rows with >= 1000 back links in a batch: %llu visits, %llu records of which %llu applied; per visit "
                        "%.1f us in all = sort %.1f + scan %.1f + gather %.1f + replay %.1f (us); heap replays (ties) %llu\n", fn,
                t.hub_rows, t.hub_records, t.hub_applied,
                t.hub_rows ? t.hub_total / 100.0 / t.hub_rows : 0.0, t.hub_rows ? t.hub_sort / 100.0 / t.hub_rows : 0.0,
                t.hub_rows ? t.hub_scan / 100.0 / t.hub_rows : 0.0, t.hub_rows ? t.hub_gather / 100.0 / t.hub_rows : 0.0,
                t.hub_rows ? t.hub_replay / 100.0 / t.hub_rows : 0.0, t.hub_ties);
    }
    return VG_OK;
}

static int32_t check_hnsw_build_args(const char *fn, int m, int ef, int max_batch, int growth_div)
{
    VG_CHECK(m >= 2 && m <= 32, VG_ERR_UNSUPPORTED, "%s: M=%d must be in 2..32 (M0 = 2M <= 64)", fn, m);
    VG_CHECK(ef >= 1 && ef <= kBuildMaxEf, VG_ERR_UNSUPPORTED, "%s: ef_construction=%d must be in 1..%d", fn, ef, kBuildMaxEf);
    VG_CHECK(max_batch >= 1 && growth_div >= 1, VG_ERR_INVALID_ARG, "%s: max_batch and growth_div must be >= 1", fn);
    return VG_OK;
}

static int32_t check_plan(const char *fn, const HnswBuildPlan &p, int max_batch)
{
    const int64_t n = p.n_old + p.count;
    VG_CHECK(p.total_rows < (int64_t(1) << 32) - 1, VG_ERR_UNSUPPORTED, "%s: too many rows", fn);
    // visited bitmaps: one per node of a batch, at most 4 GiB — larger batches are not worth more
    VG_CHECK(p.max_b * ((n + 31) / 32) * 4 <= (int64_t(1) << 32), VG_ERR_UNSUPPORTED,
             "%s: max_batch=%d needs more than 4 GiB of visited bitmaps at %lld rows", fn, max_batch, static_cast<long long>(n));
    return VG_OK;
}

// The one hand-over of a built or grown graph to the index, in vg_index_set_hnsw_graph's layout, once the stream is
// idle.  Each array replaces what the index held; one passed as the index's own (grown in place) stays.  l0c / adjc:
// the cached distances for the next vg_hnsw_insert, or null (the index then keeps none).  Edge distances uploaded for
// the older lists go: the predicate-aware walk recomputes them (same values).  Tombstones are no part of it, on
// purpose: vg_hnsw_build leaves d_hnsw_tomb as it was, vg_hnsw_insert has grown it already.
// vg_index_set_hnsw_graph does not come through here: it frees every older array BEFORE it allocates the next, and a
// failure half way leaves what it had replaced by then.
static void adopt_hnsw_graph(vg_index *idx, uint32_t *l0, float *l0c, uint32_t *slot, uint32_t *adj, float *adjc,
                             int64_t *level_off, int m, const HnswBuildPlan &p)
{
    auto put = [](auto **held, auto *fresh) {
        if (*held != fresh) drop_device(held);
        *held = fresh;
    };
    put(&idx->d_hnsw_l0, l0);
    put(&idx->d_hnsw_l0_cdist, l0c);
    put(&idx->d_hnsw_slot, slot);
    put(&idx->d_hnsw_adj, adj);
    put(&idx->d_hnsw_adj_cdist, adjc);
    put(&idx->d_hnsw_level_off, level_off);
    drop_device(&idx->d_hnsw_l0_dist);
    idx->hnsw_m0 = 2 * m;
    idx->hnsw_m = m;
    idx->hnsw_max_level = p.top;
    idx->hnsw_entry = p.entry;
}

}  // namespace vg

VG_API int32_t vg_hnsw_level_for_id(uint64_t id, int32_t m)
{
    return vg::level_for_id(id, 1.0 / std::log(static_cast<double>(m < 2 ? 2 : m)));
}

VG_API int32_t vg_hnsw_build(vg_index *idx, int32_t m, int32_t ef_construction, int32_t max_batch,
                             int32_t growth_div, void *stream)
{
    const char *fn = "vg_hnsw_build";
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(idx->d_vectors && idx->n > 0, VG_ERR_NOT_READY, "%s: index has no fp32 vectors", fn);
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    VG_TRY(vg::check_hnsw_build_args(fn, m, ef_construction, max_batch, growth_div));
    VG_CHECK(idx->n < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "%s: at most 2^31 rows", fn);
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int64_t n = idx->n;
    const int m0 = 2 * m;  // mmax0Multiplier hnsw.go:28

    // levels, slots, and what every node's insert will see as the top level: all known up front (vg_build_plan.hpp).
    // The plan's slot table is [top][n], the index's own layout: it is uploaded as it stands.
    const vg::HnswBuildPlan plan = vg::plan_hnsw_build(0, n, m, max_batch, growth_div, 0, 0, {});
    VG_TRY(vg::check_plan(fn, plan, max_batch));
    const int64_t upper_rows = plan.upper_rows, total_rows = plan.total_rows;
    const int64_t total_slots = n * m0 + upper_rows * m;

    // the graph with its build state for every row, and the batches' scratch: the call's own, not the context arena's,
    // which would keep gigabytes of it for the life of the context
    vg::DevBuf<uint32_t> d_ids, d_slots;
    vg::DevBuf<float> d_dist;
    vg::DevBuf<uint64_t> d_bits;
    vg::DevBuf<int32_t> d_cnt;
    vg::DevBuf<uint8_t> d_good;
    vg::DevBuf<int64_t> d_level_off;
    vg::DevBuf<char> scratch;
    VG_TRY(d_ids.alloc(static_cast<size_t>(total_slots)));
    VG_TRY(d_dist.alloc(static_cast<size_t>(total_slots)));
    VG_TRY(d_bits.alloc(static_cast<size_t>(total_slots)));
    VG_TRY(d_cnt.alloc(static_cast<size_t>(total_rows)));
    VG_TRY(d_good.alloc(static_cast<size_t>(total_rows)));
    VG_TRY(d_slots.alloc(plan.slots.size()));
    VG_TRY(d_level_off.alloc(plan.level_off.size()));
    vg::BuildGraph g{idx->d_vectors, n, idx->dim, idx->metric, m0, m, d_ids.p, d_ids.p + n * m0, d_dist.p, d_bits.p,
                     d_cnt.p, d_good.p, d_slots.p, d_level_off.p, nullptr, nullptr, nullptr};
    vg::BuildRun run{};
    run.ef = ef_construction;
    VG_TRY(scratch.alloc(vg::carve_run(nullptr, plan, m0, false, run, g)));
    vg::carve_run(scratch.p, plan, m0, false, run, g);
    VG_HIP(hipMemsetAsync(d_ids.p, 0xFF, static_cast<size_t>(total_slots) * 4, st));
    VG_HIP(hipMemsetAsync(d_dist.p, 0, static_cast<size_t>(total_slots) * 4, st));
    VG_HIP(hipMemsetAsync(d_bits.p, 0, static_cast<size_t>(total_slots) * 8, st));
    VG_HIP(hipMemsetAsync(d_cnt.p, 0, static_cast<size_t>(total_rows) * 4, st));
    VG_HIP(hipMemsetAsync(d_good.p, 0, static_cast<size_t>(total_rows), st));
    VG_HIP(hipMemcpyAsync(d_slots.p, plan.slots.data(), plan.slots.size() * 4, hipMemcpyHostToDevice, st));
    VG_HIP(hipMemcpyAsync(d_level_off.p, plan.level_off.data(), plan.level_off.size() * 8, hipMemcpyHostToDevice, st));
    VG_TRY(vg::run_batches(idx->ctx, st, g, plan, run, fn));

    // the index's arrays are allocated and filled BEFORE the index lets go of its previous graph: an allocation that
    // fails here (the build's own scratch is still held) leaves the previous graph searchable, metadata and all
    vg::DevBuf<uint32_t> l0, adj;
    vg::DevBuf<float> l0c, adjc;  // the cached distances, for vg_hnsw_insert
    VG_TRY(l0.alloc(static_cast<size_t>(n) * m0));
    VG_TRY(adj.alloc(static_cast<size_t>(upper_rows) * m));
    VG_TRY(l0c.alloc(static_cast<size_t>(n) * m0));
    VG_TRY(adjc.alloc(static_cast<size_t>(upper_rows) * m));
    VG_HIP(hipMemcpyAsync(l0.p, d_ids.p, static_cast<size_t>(n) * m0 * 4, hipMemcpyDeviceToDevice, st));
    VG_HIP(hipMemcpyAsync(l0c.p, d_dist.p, static_cast<size_t>(n) * m0 * 4, hipMemcpyDeviceToDevice, st));
    if (upper_rows) {
        VG_HIP(hipMemcpyAsync(adj.p, g.ids_up, static_cast<size_t>(upper_rows) * m * 4, hipMemcpyDeviceToDevice, st));
        VG_HIP(hipMemcpyAsync(adjc.p, d_dist.p + n * m0, static_cast<size_t>(upper_rows) * m * 4, hipMemcpyDeviceToDevice, st));
    }
    VG_HIP(hipStreamSynchronize(st));
    vg::adopt_hnsw_graph(idx, l0.release(), l0c.release(), d_slots.release(), adj.release(), adjc.release(),
                         d_level_off.release(), m, plan);
    idx->l0_cap = 0;
    return VG_OK;
}

VG_API int32_t vg_hnsw_insert(vg_index *idx, const float *rows, int64_t count, int32_t m, int32_t ef_construction,
                              int32_t max_batch, int32_t growth_div, void *stream)
{
    const char *fn = "vg_hnsw_insert";
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(count >= 0 && (count == 0 || rows), VG_ERR_INVALID_ARG, "%s: negative count or NULL rows", fn);
    const int64_t n_old = idx->n;
    VG_CHECK(n_old == 0 || (idx->d_vectors && idx->d_hnsw_l0), VG_ERR_NOT_READY,
             "%s: the index has rows but no HNSW graph (vg_hnsw_build first)", fn);
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    VG_TRY(vg::check_hnsw_build_args(fn, m, ef_construction, max_batch, growth_div));
    VG_CHECK(n_old + count < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "%s: at most 2^31 rows", fn);
    VG_CHECK(n_old == 0 || (m == idx->hnsw_m && idx->hnsw_m0 == 2 * m), VG_ERR_INVALID_ARG,
             "%s: M=%d does not match the graph's (M=%d, M0=%d)", fn, m, idx->hnsw_m, idx->hnsw_m0);
    const char *held = vg::held_segment_state(idx);
    VG_CHECK(!held, VG_ERR_UNSUPPORTED, "%s: the index holds %s, which the new rows would lack (segment state, "
             "not a memtable's)", fn, held);
    if (count == 0) return VG_OK;
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int64_t n_new = n_old + count;
    const int dim = idx->dim;
    const int m0 = 2 * m;

    // ---- the plan: levels, slots of the new nodes, batches (host) ----
    const int l_old = n_old ? idx->hnsw_max_level : 0;
    std::vector<int64_t> old_off(static_cast<size_t>(l_old) + 1, 0);
    if (l_old > 0) {
        VG_HIP(hipMemcpyAsync(old_off.data(), idx->d_hnsw_level_off, old_off.size() * 8, hipMemcpyDeviceToHost, st));
        VG_HIP(hipStreamSynchronize(st));
    }
    const vg::HnswBuildPlan plan = vg::plan_hnsw_build(n_old, count, m, max_batch, growth_div, idx->hnsw_entry, l_old, old_off);
    VG_TRY(vg::check_plan(fn, plan, max_batch));
    const std::vector<int64_t> &new_off = plan.level_off;
    const int l_new = plan.top;
    const int64_t upper_rows = plan.upper_rows;

    // ---- the rows and everything sized by n ----
    vg::DevIn<float> in;
    VG_TRY(in.init(rows, static_cast<size_t>(count) * dim, st));
    VG_TRY(vg::append_index_rows(idx, in.ptr, count, st));
    if (idx->d_hnsw_tomb) {  // the new rows are live
        VG_TRY(vg::grow_rows(&idx->d_hnsw_tomb, &idx->tomb_cap, n_old, n_new,
                             [](int64_t r) { return static_cast<size_t>((r + 7) / 8); }, st));
        const int64_t bytes = (n_new + 7) / 8 - n_old / 8;
        VG_LAUNCH(vg::clear_bits_kernel, dim3(static_cast<unsigned>((bytes + 255) / 256)), dim3(256), 0, st, idx->d_hnsw_tomb,
                  n_old, n_new);
    }
    // the cached distances go on with the graph when the index has them (a graph it built), or the call starts the graph
    const bool keep_cd = n_old == 0 || (idx->d_hnsw_l0_cdist && (l_old == 0 || idx->d_hnsw_adj_cdist));
    {
        int64_t cap = idx->l0_cap, cap_c = idx->l0_cap;
        VG_TRY(vg::grow_rows(&idx->d_hnsw_l0, &cap, n_old, n_new, [&](int64_t r) { return static_cast<size_t>(r) * m0 * 4; }, st));
        if (keep_cd)
            VG_TRY(vg::grow_rows(&idx->d_hnsw_l0_cdist, &cap_c, n_old, n_new,
                                 [&](int64_t r) { return static_cast<size_t>(r) * m0 * 4; }, st));
        idx->l0_cap = keep_cd ? std::min(cap, cap_c) : cap;
    }
    VG_HIP(hipMemsetAsync(idx->d_hnsw_l0 + n_old * m0, 0xFF, static_cast<size_t>(count) * m0 * 4, st));

    // ---- the upper levels re-laid for n_new nodes (the index's, swapped in at the end) ----
    vg::DevBuf<uint32_t> slots, adj;
    vg::DevBuf<float> adjc;
    vg::DevBuf<int64_t> level_off;
    VG_TRY(slots.alloc(static_cast<size_t>(l_new) * n_new));
    VG_TRY(adj.alloc(static_cast<size_t>(upper_rows) * m));
    if (keep_cd) VG_TRY(adjc.alloc(static_cast<size_t>(upper_rows) * m));
    VG_TRY(level_off.alloc(new_off.size()));
    VG_HIP(hipMemcpyAsync(level_off.p, new_off.data(), new_off.size() * 8, hipMemcpyHostToDevice, st));
    VG_HIP(hipMemsetAsync(adj.p, 0xFF, static_cast<size_t>(upper_rows) * m * 4, st));
    for (int l = 0; l < l_old; l++)
        if (old_off[l + 1] > old_off[l]) {
            VG_HIP(hipMemcpyAsync(adj.p + new_off[l] * m, idx->d_hnsw_adj + old_off[l] * m,
                                  static_cast<size_t>(old_off[l + 1] - old_off[l]) * m * 4, hipMemcpyDeviceToDevice, st));
            if (keep_cd)
                VG_HIP(hipMemcpyAsync(adjc.p + new_off[l] * m, idx->d_hnsw_adj_cdist + old_off[l] * m,
                                      static_cast<size_t>(old_off[l + 1] - old_off[l]) * m * 4, hipMemcpyDeviceToDevice, st));
        }

    // ---- per-call scratch, on the context arena: the batches' and the state rows', then the plan's slot table ----
    vg::BuildGraph g{idx->d_vectors, n_new, dim, idx->metric, m0, m, idx->d_hnsw_l0, adj.p, nullptr, nullptr, nullptr, nullptr,
                     slots.p, level_off.p, nullptr, nullptr, nullptr};
    vg::BuildRun run{};
    run.ef = ef_construction;
    run.l0_dist = idx->d_hnsw_l0_dist;
    run.dist_rows = idx->d_hnsw_l0_dist ? n_old : 0;
    run.cd0 = keep_cd ? idx->d_hnsw_l0_cdist : nullptr;
    run.cdu = keep_cd ? adjc.p : nullptr;
    vg::ArenaCall ar(idx->ctx, st);
    const int a_run = ar.add(vg::carve_run(nullptr, plan, m0, true, run, g)), a_fresh = ar.add(plan.slots.size() * 4);
    VG_TRY(ar.commit());
    vg::carve_run(ar.get<char>(a_run), plan, m0, true, run, g);
    // The plan's table holds the new nodes only ([l_new][count]); the index's holds every node: the older nodes' slots
    // are merged in on the device.  (vg_hnsw_build needs no such step: with no older nodes the two tables are one.)
    if (l_new > 0) {
        uint32_t *d_fresh = ar.get<uint32_t>(a_fresh);
        VG_HIP(hipMemcpyAsync(d_fresh, plan.slots.data(), plan.slots.size() * 4, hipMemcpyHostToDevice, st));
        const int64_t e = static_cast<int64_t>(l_new) * n_new;
        VG_LAUNCH(vg::slot_relayout_kernel, dim3(static_cast<unsigned>((e + 255) / 256)), dim3(256), 0, st, idx->d_hnsw_slot,
                  n_old, l_old, d_fresh, n_new, l_new, slots.p);
    }
    VG_TRY(vg::run_batches(idx->ctx, st, g, plan, run, fn));
    if (keep_cd && run.n_state > 0) {
        VG_LAUNCH(vg::state_writeback_kernel, dim3(static_cast<unsigned>(run.n_state)), dim3(64), 0, st, g, run.s_next,
                  run.s_first, idx->d_hnsw_l0_cdist, adjc.p);
        VG_HIP(hipStreamSynchronize(st));
    }
    if (run.totals) {
        unsigned int h[2] = {0, 0};
        VG_HIP(hipMemcpy(h, run.s_next, sizeof h, hipMemcpyDeviceToHost));
        fprintf(stderr, "%s: %lld rows, %lld batches, %u rows' build state derived\n", fn, static_cast<long long>(count),
                static_cast<long long>(plan.batches.size()), h[1]);
    }

    // ---- hand over: the layer-0 tables were grown in place; the upper levels are swapped in ----
    vg::adopt_hnsw_graph(idx, idx->d_hnsw_l0, keep_cd ? idx->d_hnsw_l0_cdist : nullptr, slots.release(), adj.release(),
                         keep_cd ? adjc.release() : nullptr, level_off.release(), m, plan);
    idx->n = n_new;
    return VG_OK;
}

VG_API int32_t vg_index_get_hnsw_graph(const vg_index *idx, int32_t *m0, int32_t *m, int32_t *max_level,
                                       uint32_t *entry_point, int64_t *level_rows, uint32_t *l0,
                                       uint32_t *upper_slot, uint32_t *upper_adj, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_get_hnsw_graph: NULL index");
    VG_CHECK(idx->d_hnsw_l0, VG_ERR_NOT_READY, "vg_index_get_hnsw_graph: index has no HNSW graph");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int L = idx->hnsw_max_level;
    std::vector<int64_t> off(static_cast<size_t>(L) + 1, 0);
    if (L > 0)
        VG_HIP(hipMemcpyAsync(off.data(), idx->d_hnsw_level_off, off.size() * 8, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    if (m0) *m0 = idx->hnsw_m0;
    if (m) *m = idx->hnsw_m;
    if (max_level) *max_level = L;
    if (entry_point) *entry_point = idx->hnsw_entry;
    if (level_rows)
        for (int l = 0; l < L; l++) level_rows[l] = off[l + 1] - off[l];
    if (l0)
        VG_HIP(hipMemcpyAsync(l0, idx->d_hnsw_l0, static_cast<size_t>(idx->n) * idx->hnsw_m0 * 4, hipMemcpyDefault, st));
    if (upper_slot && L > 0)
        VG_HIP(hipMemcpyAsync(upper_slot, idx->d_hnsw_slot, static_cast<size_t>(L) * idx->n * 4, hipMemcpyDefault, st));
    if (upper_adj && L > 0)
        VG_HIP(hipMemcpyAsync(upper_adj, idx->d_hnsw_adj, static_cast<size_t>(off[L]) * idx->hnsw_m * 4,
                              hipMemcpyDefault, st));
    VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}
