// vg_group_records.hpp — the records of a batch grouped by the row they target: the back links of the HNSW build
// and insert (k_hnsw_build.hip) and the back edges of the two Vamana builders (k_vamana_build.hip, k_vamana_fresh.hip,
// through VamanaBatch::reverse_edges, vg_vamana_common.hpp).  Per batch: rcnt[row] = the row's
// records, work[0 .. nwork) = the rows that have any, roff[row] = where the row's records start in the grouped order.
// The builders' own fill kernels (the Vamana builders share group_fill_index_kernel) then place every record's payload at
// roff[row] + (rfill[row]++), and their link kernels take one target row per workgroup and leave rcnt / rfill zero for
// the next batch.
#pragma once

#include "vg_internal.hpp"

namespace vg {

struct GroupCounters {
    unsigned int nwork, total;
};

// Both kernels append to ONE counter: a per-thread atomicAdd on it would serialise ~400 k atomics per batch on one
// L2 line (measured: most of the back-link stage).  The lanes of a wave are counted with a ballot / summed with a
// shuffle scan and the wave does one atomicAdd.
// rec_row[r] = the row record r targets, VG_INVALID_ID = no record
static __global__ void group_count_kernel(const uint32_t *__restrict__ rec_row, int64_t nrec, int32_t *__restrict__ rcnt,
                                          uint32_t *__restrict__ work, GroupCounters *__restrict__ ctr)
{
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t row = VG_INVALID_ID;
    if (r < nrec) row = rec_row[r];
    const bool first = row != VG_INVALID_ID && atomicAdd(&rcnt[row], 1) == 0;  // the row's first record this batch
    const uint64_t m = __ballot(first);
    if (m == 0) return;
    unsigned int base = 0;
    if (lane == __builtin_ctzll(m)) base = atomicAdd(&ctr->nwork, static_cast<unsigned int>(__popcll(m)));
    base = __shfl(base, __builtin_ctzll(m));
    if (first) work[base + __popcll(m & ((1ull << lane) - 1))] = row;
}

static __global__ void group_offsets_kernel(const uint32_t *__restrict__ work, const int32_t *__restrict__ rcnt,
                                            uint32_t *__restrict__ roff, GroupCounters *__restrict__ ctr)
{
    const unsigned int w = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = w < ctr->nwork;
    const uint32_t row = live ? work[w] : 0;
    const unsigned int mine = live ? static_cast<unsigned int>(rcnt[row]) : 0u;
    unsigned int incl = mine;  // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const unsigned int total = __shfl(incl, 63);
    if (total == 0) return;
    unsigned int base = 0;
    if (lane == 63) base = atomicAdd(&ctr->total, total);
    base = __shfl(base, 63);
    if (live) roff[row] = base + incl - mine;
}

// max_work: how many rows the nrec records can target at most (work has room for that many)
static int32_t group_count_offsets(const uint32_t *rec_row, int64_t nrec, int64_t max_work, int32_t *rcnt, uint32_t *work,
                                   uint32_t *roff, GroupCounters *ctr, hipStream_t st)
{
    VG_HIP(hipMemsetAsync(ctr, 0, sizeof(GroupCounters), st));
    VG_LAUNCH(group_count_kernel, dim3(static_cast<unsigned>((nrec + 255) / 256)), dim3(256), 0, st, rec_row, nrec, rcnt, work, ctr);
    VG_LAUNCH(group_offsets_kernel, dim3(static_cast<unsigned>((max_work + 255) / 256)), dim3(256), 0, st, work, rcnt, roff, ctr);
    return VG_OK;
}

}  // namespace vg
