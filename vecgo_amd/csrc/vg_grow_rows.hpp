// vg_grow_rows.hpp — rows appended to a resident index by the memtable-style inserts (vg_hnsw_insert, vg_vamana_insert):
// device arrays that grow by capacity, and the arrays every such insert grows the same way (fp32 rows, norms, bf16 image).
#pragma once

#include "vg_internal.hpp"

namespace vg {

// room for n_new rows in a device array that holds n_old (its capacity: *cap rows, 0 = n_old), grown by half at
// least so that a run of small inserts copies the array O(log n) times; bytes(r) = its size at r rows
template <typename T, typename F>
static int32_t grow_rows(T **p, int64_t *cap, int64_t n_old, int64_t n_new, F bytes, hipStream_t st)
{
    const int64_t have = std::max(*cap, n_old);
    if (*p && n_new <= have) return VG_OK;
    const int64_t want = std::max(n_new, have + have / 2);
    DevBuf<char> q;
    VG_TRY(q.alloc(bytes(want)));
    if (*p && n_old) VG_HIP(hipMemcpyAsync(q.p, *p, bytes(n_old), hipMemcpyDeviceToDevice, st));
    VG_HIP(hipStreamSynchronize(st));
    drop_device(p);
    *p = reinterpret_cast<T *>(q.release());
    *cap = want;
    return VG_OK;
}

// rows (device, count * dim fp32) become rows n_old .. n_old+count-1 of the index: the fp32 rows and their norms, the
// bf16 filter image if enabled; idx->n is the caller's to set once its graph has grown too
static int32_t append_index_rows(vg_index *idx, const float *rows, int64_t count, hipStream_t st)
{
    const int64_t n_old = idx->n, n_new = n_old + count;
    const int dim = idx->dim;
    if (!idx->d_norm_max) {
        VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_norm_max), 2 * sizeof(float)));
        VG_HIP(hipMemsetAsync(idx->d_norm_max, 0, 2 * sizeof(float), st));
    }
    if (!idx->d_flat_stats) {
        VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_flat_stats), 4 * sizeof(unsigned long long)));
        VG_HIP(hipMemsetAsync(idx->d_flat_stats, 0, 4 * sizeof(unsigned long long), st));
    }
    {
        int64_t cap = idx->rows_cap;
        VG_TRY(grow_rows(&idx->d_norms, &cap, n_old, n_new, [](int64_t r) { return static_cast<size_t>(r) * 4; }, st));
        int64_t cap_v = idx->rows_cap;
        VG_TRY(grow_rows(&idx->d_vectors, &cap_v, n_old, n_new, [&](int64_t r) { return static_cast<size_t>(r) * dim * 4; }, st));
        idx->rows_cap = std::min(cap, cap_v);
    }
    VG_HIP(hipMemcpyAsync(idx->d_vectors + n_old * dim, rows, static_cast<size_t>(count) * dim * 4, hipMemcpyDeviceToDevice, st));
    VG_TRY(append_row_norms(idx, n_old, n_new, st));
    if (idx->d_vectors_bf16) {
        const int64_t bd = idx->vectors_bf16_dim;
        VG_TRY(grow_rows(&idx->d_vectors_bf16, &idx->bf16_cap, n_old, n_new, [&](int64_t r) { return static_cast<size_t>(r) * bd * 2; }, st));
        VG_TRY(append_bf16_rows(idx, n_old, n_new, st));
    }
    return VG_OK;
}

}  // namespace vg
