// vg_vamana_common.hpp — what the Vamana builders' kernels share (k_vamana_build.hip: the DiskANN writer's buildGraph;
// k_vamana_fresh.hip: the FreshVamana insert and search): the distance of a pair of rows and its sort key, and the fill
// of their edge records once vg_group_records.hpp has grouped them.
#pragma once

#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_internal.hpp"

namespace vg {

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

}  // namespace vg
