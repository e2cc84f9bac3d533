// vg_hnsw_layer.hpp — one wavefront's walk over one HNSW layer, shared by the query kernel (k_graph.hip) and
// the builder (k_hnsw_build.hip):
//   greedy_layer   the `for changed` loop of greedySearch / insertNode    (hnsw.go:1897-1934, :918-934)
//   search_layer   searchLayerUnfiltered                                 (hnsw.go:1220-1396)
// The heaps are the reference's (vg_heap.hpp), executed uniformly by the wave on arrays the caller owns
// (LDS; for large ef SPLIT between LDS and HBM scratch, vg_heap.hpp); the <= 64 neighbours of a popped node are visited-tested, gathered
// and scored in parallel by the caller's scorer (vg_node_score.hpp: F32ScorerT, PqScorerT), then fed
// to the heaps in the node's stored neighbour order.
#pragma once

#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "../../include/vecgo_hip.h"
#include "vg_heap.hpp"
#include "vg_node_score.hpp"

namespace vg {

struct LayerStats {
    int64_t visited = 0, dc = 0, sc = 0, pops = 0;
#ifdef VG_WALK_TIMING  // stage probe (tools/build_variant.sh): s_memtime cycles per phase, reported in the stats columns
    int64_t t_pop = 0, t_adj = 0, t_score = 0, t_push = 0, t_cand = 0, t_res = 0, n_push = 0;
#endif
};
#ifdef VG_WALK_TIMING
#define VG_T(var) const int64_t var = static_cast<int64_t>(__builtin_readcyclecounter())
#define VG_TACC(acc, a, b) (acc) += (b) - (a)
#else
#define VG_T(var)
#define VG_TACC(acc, a, b)
#endif

// greedy descent on one layer: repeat { for each neighbour in list order: if nextDist < currDist take it }
// until a pass changes nothing.  row_of(node) -> the node's list on this layer (deg ids, 0xFFFFFFFF ends
// it) or nullptr.  nb_pair: 64 floats of LDS.
template <typename Scorer, typename RowFn>
__device__ __forceinline__ void greedy_layer(const Scorer &sc, int lane, RowFn row_of, int deg, float *nb_pair,
                                             float *nb_bnd, uint32_t &cur, float &cur_d, int64_t *scored = nullptr)
{
    bool changed = true;
    while (changed) {
        changed = false;
        const uint32_t *nbp = row_of(cur);
        if (nbp == nullptr) break;
        const uint32_t id_lane = lane < deg ? nbp[lane] : VG_INVALID_ID;
        const uint64_t inval = __ballot(id_lane == VG_INVALID_ID);
        const int count = inval ? __builtin_ctzll(inval) : 64;
        uint64_t mask = count >= 64 ? ~0ull : ((1ull << count) - 1);
        if (scored) *scored += count;
        sc.many(mask, id_lane, lane, nb_pair, nb_bnd);
        Scorer::sync();
        // sequential `if nextDist < currDist` over the list == the smallest distance, first of its equals, if it
        // is below currDist: a wave minimum and one ballot instead of `count` dependent LDS reads
        // (lanes past the list, and NaN distances, stand as +Inf: neither can ever be `< currDist`.  r04 padded with
        // MaxFloat32: against a list of +Inf distances — an Inf in the query — the minimum was then the PADDING, no lane
        // held it, and the lane index taken from an empty ballot read a wild neighbour id: a memory fault)
        const float raw_d = lane < count ? nb_pair[lane] : INFINITY;
        const float my_d = raw_d == raw_d ? raw_d : INFINITY;
        float mn = my_d;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float other = __shfl_xor(mn, o);
            mn = other < mn ? other : mn;
        }
        float best_d = cur_d;
        uint32_t best_id = cur;
        if (count > 0 && mn < cur_d) {  // mn is finite here: some lane of the list holds it
            const uint64_t at = __ballot(lane < count && my_d == mn);
            const int first = __builtin_ctzll(at);
            best_d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_d), first));  // its own bits (-0 == +0)
            best_id = static_cast<uint32_t>(__builtin_amdgcn_readlane(id_lane, first));
            changed = true;
        }
        cur = best_id;
        cur_d = best_d;
        Scorer::sync();
    }
}

// searchLayerUnfiltered from (ep, ep_d).  `vis`: this wave's visited bitmap, already clear.  On return
// res[0..res_len) is the results max-heap exactly as the reference's search leaves it.
// UK: every distance is >= +0 (any metric but Dot), see heap_sift_down_uk (vg_heap.hpp)
// NaN distances (a NaN or an Inf in a row or in the query).  Every comparison with a NaN is FALSE in the reference
// (queue.go:75-82,199-203; hnsw.go:1376 `nextDist > bound`), which this walk relies on NOT happening in two places: the
// unsigned-key sifts order a NaN's bit pattern as the largest key, and the neighbour loop rejects every lane above the
// bound at once because "the bound only falls" — with a NaN inside the results heap a sift-down can bring it to the
// root, and against a NaN bound nothing is rejected any more.  So:
//   `odd_out` != nullptr  one ballot over each scored neighbour list watches for a distance that is a NaN (UK: any bit
//                         pattern above +Inf's, which covers negative values too); at the first one the walk stops with
//                         *odd_out = true, and the caller runs the query again, with UK = false and
//   STRICT                every lane tested against the bound at ITS turn, as the reference's loop is written.
// nullptr / false: the fast form (the builder, and every query that meets no NaN).
template <bool UK = false, bool STRICT = false, typename Scorer, typename RowFn, typename Heap>
__device__ __forceinline__ void search_layer(const Scorer &sc, bool l2_metric, int lane, RowFn row_of, int deg,
                                             uint32_t ep, float ep_d, int ef, Heap cand, Heap res,
                                             float *nb_pair, float *nb_bnd, uint32_t *vis, int &res_len_out,
                                             LayerStats &st, bool *odd_out = nullptr, const uint8_t *dead = nullptr)
{
    // dead (STRICT instances only): g.tombstones as a bitmap — a deleted node goes to the exploration queue like any other but
    // never to the results, and so never moves the bound (hnsw.go:1381-1390; entry point :1559-1565)
    constexpr bool strict = STRICT;
    auto is_odd = [](float d) { return UK ? __float_as_uint(d) > 0x7F800000u : d != d; };
    if (odd_out && is_odd(ep_d)) {  // wave-uniform
        *odd_out = true;
        res_len_out = 0;
        return;
    }
    int cand_len = 0, res_len = 0;
    if (lane == 0) atomicOr(&vis[ep >> 5], 1u << (ep & 31));
    heap_push<false>(cand, cand_len, HItem{ep, ep_d});
    if (!(STRICT && dead && mask_bit(dead, ep))) heap_push<true>(res, res_len, HItem{ep, ep_d});
    const bool use_sc = Scorer::kBounded && l2_metric;
    int cap = ef * 2;
    int stagnant = 0;
    float last_best = 3.40282346638528859811704183484516925440e+38f;
    const int min_cap = ef + ef * 3 / 4;
    Scorer::sync();

    while (cand_len > 0) {
        VG_T(t0);
        const HItem c = heap_pop<false, UK>(cand, cand_len);
        st.pops++;
        if (res_len > 0) {
            const float worst = heap_get(res, 0).dist;
            if (c.dist > worst && res_len >= ef) break;
            if (worst < last_best * 0.999f) {
                last_best = worst;
                stagnant = 0;
            } else if (res_len >= ef) {
                stagnant++;
                if (stagnant >= 8 && cap > min_cap) {
                    cap -= ef / 8;
                    if (cap < min_cap) cap = min_cap;
                    stagnant = 0;
                }
            }
        }
        VG_T(t1);
        const uint32_t *nbp = row_of(c.node);
        const uint32_t id_lane = (nbp != nullptr && lane < deg) ? nbp[lane] : VG_INVALID_ID;
        const uint64_t inval = __ballot(id_lane == VG_INVALID_ID);
        const int count = inval ? __builtin_ctzll(inval) : 64;
        // CheckAndVisit for the whole list at once (neighbour ids of a node are distinct)
        // (a returning L2 atomic: a plain load could hit a stale L1 line of this very bitmap)
        bool fresh = false;
        if (lane < count) {
            const uint32_t bit = 1u << (id_lane & 31);
            fresh = (atomicOr(&vis[id_lane >> 5], bit) & bit) == 0;
        }
        const uint64_t newmask = __ballot(fresh);
        uint64_t deadmask = 0;
        if constexpr (STRICT) {
            if (dead) deadmask = __ballot(fresh && mask_bit(dead, id_lane));
        }
        st.visited += __popcll(newmask);
        VG_T(t2);
        sc.many(newmask, id_lane, lane, nb_pair, nb_bnd);
        Scorer::sync();
        // lane j keeps node j's two distances; the loop below reads them with readlane, not from LDS
        const float my_pair = nb_pair[lane];
        const float my_nd = use_sc ? nb_bnd[lane] : my_pair;  // what the reference compares once a bound exists
        if (odd_out && __ballot(((newmask >> lane) & 1) && (is_odd(my_pair) || is_odd(my_nd)))) {
            *odd_out = true;
            res_len_out = 0;
            return;
        }
        VG_T(t3);
        bool has_bound = res_len >= ef;
        float bound = has_bound ? heap_get(res, 0).dist : 0.0f;
        uint64_t todo = newmask;
        uint64_t accepted = 0, pre_bound = 0;
        st.dc += __popcll(newmask);
        // the heap updates are one wave's dependent chain: let it issue ahead of the waves that are scoring (3-4 % on
        // the PQ walk at ef <= 512, nothing elsewhere)
        __builtin_amdgcn_s_setprio(3);
        while (todo) {
            if (has_bound && !strict) {
                // the bound only falls: a node above it now is above it at its turn (SquaredL2Bounded reports
                // exceeded, or `nd > bound` skips it)
                const uint64_t rej = __ballot(my_nd > bound) & todo;
                if (use_sc) st.sc += __popcll(rej);
                todo &= ~rej;
                if (!todo) break;
            }
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t id = static_cast<uint32_t>(__builtin_amdgcn_readlane(id_lane, j));
            const float nd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(has_bound ? my_nd : my_pair), j));
            if (strict && has_bound && nd > bound) {  // at its turn, against the bound as it stands now
                if (use_sc) st.sc++;
                continue;
            }
            VG_T(tc0);
            accepted |= 1ull << j;  // its candidates-heap push happens after the loop (the two heaps are independent)
            if (!has_bound) pre_bound |= 1ull << j;  // pushed with the SquaredL2 value, not the bounded kernel's
            if (STRICT && ((deadmask >> j) & 1)) continue;  // tombstoned: the exploration queue only
            VG_T(tc1);
            if (has_bound) {  // results heap full: its top is `bound`
                res_replace_top<UK>(res, res_len, HItem{id, nd}, bound);
            } else {
                res_push_bounded<UK>(res, res_len, HItem{id, nd}, ef);
                if (res_len >= ef) {
                    bound = heap_get(res, 0).dist;
                    has_bound = true;
                }
            }
            VG_T(tc2);
            VG_TACC(st.t_cand, tc0, tc1);
            VG_TACC(st.t_res, tc1, tc2);
#ifdef VG_WALK_TIMING
            st.n_push++;
#endif
        }
        // TryPushBounded of the accepted nodes, in neighbour order (what the reference interleaves with the results
        // heap's updates; neither heap reads the other).  While the heap is below its cap they are plain pushes: one run
        // (heap_push_run_min); at the cap each one is the replace-the-closest path.
        if (accepted) {
            const float acc_d = ((pre_bound >> lane) & 1) ? my_pair : my_nd;  // the value the node was accepted with
            int fit = cap - cand_len;
            fit = fit < 0 ? 0 : fit;
            uint64_t run = accepted, rest = 0;
            if (__popcll(accepted) > fit) {
                run = 0;
                uint64_t a = accepted;
                for (int c = 0; c < fit; c++) {
                    run |= a & (~a + 1);
                    a &= a - 1;
                }
                rest = a;
            }
            heap_push_run_min(cand, cand_len, run, id_lane, acc_d);
            while (rest) {
                const int j = __builtin_ctzll(rest);
                rest &= rest - 1;
                cand_try_push_bounded<UK>(cand, cand_len,
                                          HItem{static_cast<uint32_t>(__builtin_amdgcn_readlane(id_lane, j)),
                                                __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc_d), j))}, cap);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        Scorer::sync();
        VG_T(t4);
        VG_TACC(st.t_pop, t0, t1);
        VG_TACC(st.t_adj, t1, t2);
        VG_TACC(st.t_score, t2, t3);
        VG_TACC(st.t_push, t3, t4);
    }
    res_len_out = res_len;
}

// The results heap's items in ascending order without popping them: a sort of a copy (`keys`: the finished candidates
// heap's LDS, 2 * ef items >= the next power of two of res_len; an item's 8 bytes are its key, distance bits above the
// node id — distances >= +0, UK).  Popping the heap gives the same order exactly when no two of the `check` closest
// distances are equal (ties pop in the order the heap's layout dictates) and none is a NaN: returns false then, and
// the caller pops.
__device__ __forceinline__ bool results_sorted_lds(const HItem *res, int res_len, uint64_t *keys, int check, int lane)
{
    const uint64_t *items = reinterpret_cast<const uint64_t *>(res);
    int n2 = 1;
    while (n2 < res_len) n2 <<= 1;
    bool bad = false;
    __syncthreads();
    for (int i = lane; i < n2; i += 64) {
        uint64_t key = ~0ull;
        if (i < res_len) {
            key = items[i];
            bad |= static_cast<uint32_t>(key >> 32) > 0x7F800000u;
        }
        keys[i] = key;
    }
    __syncthreads();
    bitonic_sort_lds(keys, n2, lane, 64);
    const int have = res_len < check ? res_len : check;
    for (int i = lane; i + 1 < have; i += 64) bad |= (keys[i] >> 32) == (keys[i + 1] >> 32);
    return __ballot(bad) == 0;
}

}  // namespace vg
