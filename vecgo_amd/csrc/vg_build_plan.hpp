// vg_build_plan.hpp — what the graph builders work out on the host before the first kernel: the level of every new
// node, where its upper rows go, the batch schedule and the (node, level) pairs of every batch.  All of it follows
// from the ids alone (ApplyInsert's ids are the row numbers, the levels a hash of them), so it is known up front.
// Plain C++: no HIP, the host test program includes it (the counter RNG alone is also a device function under hipcc).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define VG_HOST_DEVICE __host__ __device__
#else
#define VG_HOST_DEVICE
#endif

namespace vg {

VG_HOST_DEVICE inline uint64_t vb_splitmix64(uint64_t x)
{
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}
// vgo_rng_u64 (the oracle's counter RNG): the Vamana build's initial graph, the FreshVamana insert's entry-point draws
VG_HOST_DEVICE inline uint64_t vb_rng_u64(uint64_t seed, uint64_t a, uint64_t b, uint64_t c)
{
    uint64_t h = vb_splitmix64(seed);
    h = vb_splitmix64(h ^ a);
    h = vb_splitmix64(h ^ b);
    return vb_splitmix64(h ^ c);
}

// layerForApplyInsert (hnsw.go:2103-2116), layerMultiplier = 1 / ln(M) (hnsw.go:218)
inline int32_t level_for_id(uint64_t id, double mult)
{
    uint64_t x = id + 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    x ^= x >> 31;
    const double inv = 1.0 / 9007199254740992.0;
    double r = static_cast<double>(x >> 11) * inv;
    if (r == 0) r = inv;
    const int32_t lv = static_cast<int32_t>(std::floor(-std::log(r) * mult));
    return lv > 62 ? 62 : lv;
}

// The batch after `done` inserts of a schedule that ends at `end`: clamp(done / growth_div, 1, max_batch) nodes
// (max_batch = 1: the reference's sequential loop), never past the end
inline int64_t next_batch(int64_t done, int64_t end, int64_t max_batch, int64_t growth_div)
{
    return std::min(std::max<int64_t>(1, std::min(done / growth_div, max_batch)), end - done);
}

// purpose constant of the FreshVamana entry-point draws: rng_u64(seed, count, kFreshEntryPurpose, 0) (header, vg_vamana_insert)
constexpr uint64_t kFreshEntryPurpose = 0x4652455348ull;  // "FRESH"

// maybeUpdateEntryPoint (fresh_vamana.go:795-801) after the insert that made the graph `count` nodes: below 100 always,
// at every multiple of 500 with probability 0.1 (the draw: the top 24 bits of the counter RNG as a float32 in [0, 1))
inline bool fresh_entry_moves(int64_t count, uint64_t seed)
{
    if (count < 100) return true;
    if (count % 500 != 0) return false;
    const float u = static_cast<float>(vb_rng_u64(seed, static_cast<uint64_t>(count), kFreshEntryPurpose, 0) >> 40) * (1.0f / 16777216.0f);
    return u < 0.1f;
}

// One batch of the schedule: nodes t0 .. t0+size-1, their (node, level) pairs, the entry point and top level
// their searches start from
struct BuildBatch {
    int64_t t0, size, npairs;
    uint32_t entry;
    int cur_top;
};

// Nodes n_old .. n_old+count-1 inserted into a graph of n_old nodes (vg_hnsw_build: n_old = 0).  Everything indexed
// by node is indexed from n_old on.
struct HnswBuildPlan {
    int64_t n_old = 0, count = 0;
    std::vector<int32_t> levels;     // [count]
    std::vector<uint32_t> slots;     // [top][count]: the new node's row in the level's table, VG_INVALID_ID = none
    std::vector<int64_t> level_off;  // [top + 1]: first row of every level's table after the call
    std::vector<BuildBatch> batches;
    // pair_base[i] = node n_old + i's first (node, level) pair (levels 0..min(level, top of its batch) in order);
    // pair_node / pair_level = the pairs
    std::vector<int64_t> pair_base;  // [count + 1]
    std::vector<uint32_t> pair_node;
    std::vector<int32_t> pair_level;
    int64_t max_pairs = 1, max_b = 1;  // the largest batch's, at least 1
    int64_t upper_rows = 0, total_rows = 0;
    uint32_t entry = 0;  // entry point and top level (= the number of upper levels) after the last batch
    int top = 0;
};

// old_off: the n_old nodes' level offsets (old_top + 1 entries; unused when n_old = 0).  New nodes' upper rows go at the
// end of each level's table, slots in id order: a full build's layout.
inline HnswBuildPlan plan_hnsw_build(int64_t n_old, int64_t count, int m, int64_t max_batch, int64_t growth_div,
                                     uint32_t old_entry, int old_top, const std::vector<int64_t> &old_off)
{
    HnswBuildPlan p;
    p.n_old = n_old;
    p.count = count;
    const double mult = 1.0 / std::log(static_cast<double>(m));
    p.levels.resize(static_cast<size_t>(count));
    int new_top = 0;
    for (int64_t i = 0; i < count; i++) {
        p.levels[i] = level_for_id(static_cast<uint64_t>(n_old + i), mult);
        new_top = std::max(new_top, p.levels[i]);
    }
    const int l_old = n_old ? old_top : 0;
    const int n_levels = std::max(l_old, new_top);
    p.level_off.assign(static_cast<size_t>(n_levels) + 1, 0);
    p.slots.resize(static_cast<size_t>(n_levels) * count);
    for (int l = 0; l < n_levels; l++) {
        uint32_t next = static_cast<uint32_t>(l < l_old ? old_off[l + 1] - old_off[l] : 0);
        for (int64_t i = 0; i < count; i++)
            p.slots[static_cast<size_t>(l) * count + i] = p.levels[i] >= l + 1 ? next++ : 0xFFFFFFFFu;
        p.level_off[l + 1] = p.level_off[l] + next;
    }
    p.upper_rows = p.level_off[n_levels];
    p.total_rows = n_old + count + p.upper_rows;

    p.pair_base.assign(static_cast<size_t>(count) + 1, 0);
    p.entry = n_old ? old_entry : 0;
    p.top = n_old ? l_old : (count ? p.levels[0] : 0);
    const int64_t end = n_old + count;
    for (int64_t done = n_old ? n_old : 1; done < end;) {  // an empty graph: row 0 becomes the entry point, with no links
        BuildBatch bt{done, next_batch(done, end, max_batch, growth_div), 0, p.entry, p.top};
        for (int64_t t = done; t < done + bt.size; t++) {
            const int lt = p.levels[t - n_old];
            for (int l = 0; l <= std::min(lt, bt.cur_top); l++) {
                p.pair_node.push_back(static_cast<uint32_t>(t));
                p.pair_level.push_back(l);
            }
            p.pair_base[t - n_old + 1] = static_cast<int64_t>(p.pair_node.size());
            if (lt > p.top) {  // updateEntryPoint hnsw.go:885-900
                p.top = lt;
                p.entry = static_cast<uint32_t>(t);
            }
        }
        bt.npairs = p.pair_base[done + bt.size - n_old] - p.pair_base[done - n_old];
        p.max_pairs = std::max(p.max_pairs, bt.npairs);
        p.max_b = std::max(p.max_b, bt.size);
        p.batches.push_back(bt);
        done += bt.size;
    }
    return p;
}

// vg_vamana_insert's schedule for nodes n_old .. n_old+count-1: the batches (npairs, cur_top unused) with the entry point
// every node of a batch starts from, and the entry point after the last.  An empty graph: row 0 becomes the entry point,
// with no links, and is no batch's node.
struct FreshInsertPlan {
    std::vector<BuildBatch> batches;
    int64_t max_b = 1;
    uint32_t entry = 0;
};
inline FreshInsertPlan plan_fresh_insert(int64_t n_old, int64_t count, int64_t max_batch, int64_t growth_div, uint64_t seed,
                                         uint32_t old_entry)
{
    FreshInsertPlan p;
    p.entry = n_old ? old_entry : 0;
    const int64_t end = n_old + count;
    for (int64_t done = n_old ? n_old : 1; done < end;) {
        const BuildBatch bt{done, next_batch(done, end, max_batch, growth_div), 0, p.entry, 0};
        for (int64_t t = done; t < done + bt.size; t++)
            if (fresh_entry_moves(t + 1, seed)) p.entry = static_cast<uint32_t>(t);
        p.max_b = std::max(p.max_b, bt.size);
        p.batches.push_back(bt);
        done += bt.size;
    }
    return p;
}

}  // namespace vg
