// vg_walk_chunk.hpp — how many queries of a graph walk share one launch.  HOST ONLY (no HIP): the library's walkers use it
// through WalkChunks (vg_search.hpp), tests/cpp/host_mirror_test.cpp checks it at compile time.
#pragma once

#include <cstdint>

namespace vg {

// as many queries as `cap` bytes of scratch hold at per_query bytes each: at least one, at most the batch
constexpr int64_t walk_chunk(int64_t cap, int64_t per_query, int64_t nq)
{
    const int64_t fit = cap / (per_query > 1 ? per_query : 1);
    return fit < 1 ? 1 : fit < nq ? fit : nq;
}

}  // namespace vg
