// k_merge.hip — vg_index_merge: Engine.CompactWithContext's Iterate loop (engine/compaction.go:173-218) over resident
//               indexes.  N sources are walked in order, the rows whose bit is set in that source's tombstone bitmap are
//               skipped, the survivors are appended to one new index, and the move maps say where every row went.
//
// Four launches, whatever the rows and however many sources (a memtable flush has 16 shards, a compaction may have hundreds
// of small segments):
//   merge_count   one work block = kMergeBlockRows consecutive rows of ONE source (a lane owns one bitmap byte = 8 rows):
//                 the live rows per work block.  A work block finds its source by bisection over the descriptors' first
//                 work block, so the grid runs over the work blocks of all sources at once.
//   merge_scan    one workgroup: the exclusive prefix of those counts over all work blocks of all sources, and the total.
//                 The host reads the total (the new index's row count: capacities are exact) and allocates.
//   merge_rank    the count pass again, ranked with rb_block_scan on top of the work block's prefix: old_to_new for every
//                 source row, (source, row) for every new row.
//   merge_gather  new row j <- row new_row[j] of source new_source[j], and its norm; a row is moved by up to 64 lanes in
//                 16-, 8- or 4-byte words (dim * 4 is a multiple of 4), four words in flight per lane, with nontemporal
//                 loads and stores (every row is read once and written once; measured: DESIGN.md).  The lanes fold
//                 max |x| and max ||x||^2 of what they move: d_norm_max is recomputed (a deleted row may have held a
//                 source's maximum) without reading the new rows back.
// A norm is a function of its row alone (row_norms_kernel, k_exact.hip), so the gathered norms are vg_index_set_vectors'
// bit for bit; both maxima are order-free (non-negative floats order like their bits; a NaN norm is skipped as fmaxf skips
// it, a NaN element counts as +Inf as it does there).
#include "vg_permute.hpp"

namespace vg {
namespace {

constexpr int kMergeRowsPerLane = 8;                               // one bitmap byte: no wider load, bitmaps start at any byte
constexpr int kMergeBlockRows = kRbThreads * kMergeRowsPerLane;    // rows of one source per work block

struct MergeSource {
    const float *rows;       // n * dim
    const float *norms;      // n
    const uint8_t *deleted;  // device memory at any byte address, ceil(n / 8) bytes; null: nothing deleted
    int64_t n;
    int64_t first_block;     // the work blocks of the sources in front
    uint32_t first_row;      // the rows of the sources in front (off_s of old_to_new)
    uint32_t unused;
};

// the last source whose first work block is <= b: never an empty one, an empty source shares its first block with the next
__device__ __forceinline__ int merge_source_of(const MergeSource *__restrict__ src, int n_sources, int64_t b)
{
    int lo = 0, hi = n_sources - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (src[mid].first_block <= b)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// bit r = row row0 + r of the source is live; row0 is a multiple of 8; bits at or above n are not rows
__device__ __forceinline__ uint32_t merge_live_bits(const MergeSource &s, int64_t row0)
{
    const int64_t left = s.n - row0;
    if (left <= 0) return 0u;
    const uint32_t valid = left >= kMergeRowsPerLane ? 0xFFu : (1u << left) - 1u;
    const uint32_t dead = s.deleted ? s.deleted[row0 >> 3] : 0u;
    return ~dead & valid;
}

__global__ __launch_bounds__(kRbThreads) void merge_count_kernel(const MergeSource *__restrict__ src, int n_sources, int64_t blocks,
                                                                 uint32_t *__restrict__ block_live)
{
    __shared__ uint32_t wsum[kRbThreads / 64];
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const MergeSource s = src[merge_source_of(src, n_sources, b)];
        const int64_t row0 = (b - s.first_block) * kMergeBlockRows + static_cast<int64_t>(threadIdx.x) * kMergeRowsPerLane;
        uint32_t total;
        rb_block_scan(__popc(merge_live_bits(s, row0)), wsum, &total);
        if (threadIdx.x == 0) block_live[b] = total;
    }
}

// block_live[b] <- the live rows in front of work block b, block_live[blocks] <- all live rows; one workgroup
__global__ __launch_bounds__(kRbThreads) void merge_scan_kernel(uint32_t *__restrict__ block_live, int64_t blocks)
{
    __shared__ uint32_t wsum[kRbThreads / 64];
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < blocks; b0 += kRbThreads) {
        const int64_t b = b0 + threadIdx.x;
        uint32_t total;
        const uint32_t before = rb_block_scan(b < blocks ? block_live[b] : 0u, wsum, &total);
        if (b < blocks) block_live[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) block_live[blocks] = carry;
}

__global__ __launch_bounds__(kRbThreads) void merge_rank_kernel(const MergeSource *__restrict__ src, int n_sources, int64_t blocks,
                                                                const uint32_t *__restrict__ block_base, uint32_t live_rows,
                                                                uint32_t *__restrict__ old_to_new, int32_t *__restrict__ new_source,
                                                                uint32_t *__restrict__ new_row)
{
    __shared__ uint32_t wsum[kRbThreads / 64];
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int si = merge_source_of(src, n_sources, b);
        const MergeSource s = src[si];
        const int64_t row0 = (b - s.first_block) * kMergeBlockRows + static_cast<int64_t>(threadIdx.x) * kMergeRowsPerLane;
        const uint32_t bits = merge_live_bits(s, row0);
        uint32_t total;
        uint32_t j = block_base[b] + rb_block_scan(__popc(bits), wsum, &total);
        const int64_t left = s.n - row0;
        for (int r = 0; r < kMergeRowsPerLane && r < left; r++) {
            const bool live = (bits >> r) & 1u;
            if (old_to_new) old_to_new[static_cast<int64_t>(s.first_row) + row0 + r] = live ? j : VG_INVALID_ID;
            if (live && j < live_rows) {  // (always, unless the caller rewrites a device bitmap under the call)
                new_source[j] = si;
                new_row[j] = static_cast<uint32_t>(row0 + r);
                j++;
            }
        }
    }
}

__device__ __forceinline__ float merge_fold_abs(float mx, uint32_t word)
{
    const float a = fabsf(__uint_as_float(word));
    return fmaxf(mx, a == a ? a : INFINITY);
}
// the words a row moves in (compiler vectors: the nontemporal builtins take them, not HIP's uint2 / uint4 structs)
typedef uint32_t merge_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t merge_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float merge_max_abs(float mx, uint32_t v) { return merge_fold_abs(mx, v); }
__device__ __forceinline__ float merge_max_abs(float mx, merge_u32x2 v) { return merge_fold_abs(merge_fold_abs(mx, v.x), v.y); }
__device__ __forceinline__ float merge_max_abs(float mx, merge_u32x4 v)
{
    return merge_fold_abs(merge_fold_abs(merge_fold_abs(merge_fold_abs(mx, v.x), v.y), v.z), v.w);
}

// 1 << lane_shift lanes (at most a wave) move one row of `words` W-byte words; maxima[0] = max ||x||^2, maxima[1] = max |x|
// as the bits of non-negative floats, zero before the launch
template <typename W>
__global__ __launch_bounds__(kRbThreads) void merge_gather_kernel(const MergeSource *__restrict__ src, const int32_t *__restrict__ new_source,
                                                                  const uint32_t *__restrict__ new_row, int64_t live, int words, int lane_shift,
                                                                  W *__restrict__ dst_rows, float *__restrict__ dst_norms, int *__restrict__ maxima)
{
    const int lanes = 1 << lane_shift, k0 = threadIdx.x & (lanes - 1);
    const int64_t rows_per_block = kRbThreads >> lane_shift;
    float mx = 0.0f, nmax = 0.0f;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * rows_per_block + (threadIdx.x >> lane_shift); q < live;
         q += static_cast<int64_t>(gridDim.x) * rows_per_block) {
        const MergeSource &s = src[new_source[q]];
        const int64_t row = new_row[q];
        const W *__restrict__ from = reinterpret_cast<const W *>(s.rows) + row * words;
        W *__restrict__ to = dst_rows + q * words;
        for (int k = k0; k < words; k += 4 * lanes) {
            W v[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (k + u * lanes < words) v[u] = __builtin_nontemporal_load(from + k + u * lanes);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (k + u * lanes < words) {
                    __builtin_nontemporal_store(v[u], to + k + u * lanes);
                    mx = merge_max_abs(mx, v[u]);
                }
        }
        if (k0 == 0) {
            const float nv = s.norms[row];
            dst_norms[q] = nv;
            if (nv == nv) nmax = fmaxf(nmax, nv);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off));
        nmax = fmaxf(nmax, __shfl_xor(nmax, off));
    }
    if ((threadIdx.x & 63) == 0) {  // (the atomic only where it would raise the value: row_norms_kernel's note, k_exact.hip)
        if (__float_as_int(nmax) > *reinterpret_cast<volatile int *>(maxima)) atomicMax(maxima, __float_as_int(nmax));
        if (__float_as_int(mx) > *reinterpret_cast<volatile int *>(maxima + 1)) atomicMax(maxima + 1, __float_as_int(mx));
    }
}

// what the call stages on the host; lives until the stream has taken it
struct MergeStaged {
    std::vector<MergeSource> table;
    std::vector<uint8_t> host_bits;  // the host bitmaps one after the other
};

int32_t merge_run(vg_ctx *ctx, const vg_index *const *sources, const uint8_t *const *deleted, int32_t n_sources, int64_t total,
                  MergeStaged &hs, vg_index **merged, uint32_t *old_to_new, int32_t *new_source, uint32_t *new_row, hipStream_t st)
{
    const int32_t dim = sources[0]->dim;
    hs.table.resize(static_cast<size_t>(n_sources));
    std::vector<int64_t> host_off(static_cast<size_t>(n_sources), -1);
    int64_t blocks = 0, first_row = 0;
    for (int32_t s = 0; s < n_sources; s++) {
        const int64_t n = sources[s]->n;
        hs.table[s] = MergeSource{sources[s]->d_vectors, sources[s]->d_norms, nullptr, n, blocks, static_cast<uint32_t>(first_row), 0u};
        const uint8_t *bits = deleted ? deleted[s] : nullptr;
        if (bits && n > 0) {
            if (is_device_ptr(bits)) {
                hs.table[s].deleted = bits;
            } else {
                host_off[s] = static_cast<int64_t>(hs.host_bits.size());
                hs.host_bits.insert(hs.host_bits.end(), bits, bits + (n + 7) / 8);
            }
        }
        blocks += (n + kMergeBlockRows - 1) / kMergeBlockRows;
        first_row += n;
    }
    DevTmp<uint8_t> d_bits;
    VG_TRY(d_bits.init(hs.host_bits.size(), st));
    if (!hs.host_bits.empty()) VG_HIP(hipMemcpyAsync(d_bits.ptr, hs.host_bits.data(), hs.host_bits.size(), hipMemcpyHostToDevice, st));
    for (int32_t s = 0; s < n_sources; s++)
        if (host_off[s] >= 0) hs.table[s].deleted = d_bits.ptr + host_off[s];
    DevTmp<MergeSource> d_table;
    VG_TRY(d_table.init(hs.table.size(), st));
    VG_HIP(hipMemcpyAsync(d_table.ptr, hs.table.data(), hs.table.size() * sizeof(MergeSource), hipMemcpyHostToDevice, st));
    DevTmp<uint32_t> block_live;
    VG_TRY(block_live.init(static_cast<size_t>(blocks) + 1, st));
    DevOut<uint32_t> o2n;
    VG_TRY(o2n.init(old_to_new, static_cast<size_t>(total), st, kAnyAlign));

    const unsigned grid = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(blocks, 4096)));
    uint32_t live = 0;
    if (blocks > 0) {
        {
            ProfScope p(ctx, "merge_count", st);
            VG_LAUNCH(merge_count_kernel, dim3(grid), dim3(kRbThreads), 0, st, d_table.ptr, n_sources, blocks, block_live.ptr);
        }
        {
            ProfScope p(ctx, "merge_scan", st);
            VG_LAUNCH(merge_scan_kernel, dim3(1), dim3(kRbThreads), 0, st, block_live.ptr, blocks);
        }
        VG_HIP(hipMemcpyAsync(&live, block_live.ptr + blocks, sizeof live, hipMemcpyDeviceToHost, st));
        VG_HIP(hipStreamSynchronize(st));
    }

    // the index vg_index_create + vg_index_set_vectors leave: rows, norms, maxima and counters, or none of them at 0 rows
    VG_TRY(vg_index_create(ctx, static_cast<int64_t>(live), dim, sources[0]->metric, merged));
    vg_index *idx = *merged;
    if (live > 0) {
        VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_vectors), static_cast<size_t>(live) * dim * sizeof(float)));
        VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_norms), static_cast<size_t>(live) * sizeof(float)));
        VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_norm_max), 2 * sizeof(float)));
        VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_flat_stats), 4 * sizeof(unsigned long long)));
        VG_HIP(hipMemsetAsync(idx->d_norm_max, 0, 2 * sizeof(float), st));
        VG_HIP(hipMemsetAsync(idx->d_flat_stats, 0, 4 * sizeof(unsigned long long), st));
    }
    DevTmp<int32_t> ns;
    DevTmp<uint32_t> nr;
    VG_TRY(ns.init(live, st));
    VG_TRY(nr.init(live, st));
    if (blocks > 0) {
        ProfScope p(ctx, "merge_rank", st);
        VG_LAUNCH(merge_rank_kernel, dim3(grid), dim3(kRbThreads), 0, st, d_table.ptr, n_sources, blocks, block_live.ptr, live, o2n.ptr,
                  ns.ptr, nr.ptr);
    }
    if (live > 0) {
        const int64_t row_bytes = static_cast<int64_t>(dim) * 4;
        const int64_t w = rb_word_bytes(row_bytes);  // 16, 8 or 4: dim * 4 is a multiple of 4
        const int words = static_cast<int>(row_bytes / w);
        int lane_shift = 0;
        while (lane_shift < 6 && (1 << lane_shift) < words) lane_shift++;
        const int64_t groups = (static_cast<int64_t>(live) + (kRbThreads >> lane_shift) - 1) / (kRbThreads >> lane_shift);
        const unsigned ggrid = static_cast<unsigned>(std::min<int64_t>(groups, 8192));
        {  // (the scope times the kernel alone: it closes before the maps are copied out)
            ProfScope p(ctx, "merge_gather", st);
#define VG_MERGE_GATHER(T)                                                                                                         \
    VG_LAUNCH(merge_gather_kernel<T>, dim3(ggrid), dim3(kRbThreads), 0, st, d_table.ptr, ns.ptr, nr.ptr, static_cast<int64_t>(live), words, \
              lane_shift, reinterpret_cast<T *>(idx->d_vectors), idx->d_norms, reinterpret_cast<int *>(idx->d_norm_max))
            switch (w) {
                case 16: VG_MERGE_GATHER(merge_u32x4); break;
                case 8: VG_MERGE_GATHER(merge_u32x2); break;
                default: VG_MERGE_GATHER(uint32_t); break;
            }
#undef VG_MERGE_GATHER
        }
        if (new_source) VG_HIP(hipMemcpyAsync(new_source, ns.ptr, static_cast<size_t>(live) * sizeof(int32_t), hipMemcpyDefault, st));
        if (new_row) VG_HIP(hipMemcpyAsync(new_row, nr.ptr, static_cast<size_t>(live) * sizeof(uint32_t), hipMemcpyDefault, st));
    }
    VG_TRY(o2n.finish());
    VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}

}  // namespace
}  // namespace vg

VG_API int32_t vg_index_merge(vg_ctx *ctx, const vg_index *const *sources, const uint8_t *const *deleted, int32_t n_sources,
                              vg_index **out, uint32_t *old_to_new, int32_t *new_source, uint32_t *new_row, void *stream)
{
    if (out) *out = nullptr;
    VG_CHECK(ctx && sources && out, VG_ERR_INVALID_ARG, "vg_index_merge: NULL context, sources or result");
    VG_CHECK(n_sources >= 1, VG_ERR_INVALID_ARG, "vg_index_merge: n_sources = %d, at least one source", n_sources);
    for (int32_t s = 0; s < n_sources; s++) VG_CHECK(sources[s], VG_ERR_INVALID_ARG, "vg_index_merge: source %d is NULL", s);
    for (int32_t s = 0; s < n_sources; s++)
        VG_CHECK(sources[s]->ctx == ctx, VG_ERR_INVALID_ARG, "vg_index_merge: source %d lives on another context", s);
    for (int32_t s = 1; s < n_sources; s++) VG_CHECK(sources[s]->dim == sources[0]->dim, VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
    for (int32_t s = 1; s < n_sources; s++)
        VG_CHECK(sources[s]->metric == sources[0]->metric, VG_ERR_INVALID_ARG, "vg_index_merge: source %d has metric %d, source 0 has %d", s,
                 sources[s]->metric, sources[0]->metric);
    VG_CHECK(sources[0]->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    int64_t total = 0;
    for (int32_t s = 0; s < n_sources; s++) {
        VG_CHECK(sources[s]->n == 0 || sources[s]->d_vectors, VG_ERR_NOT_READY, "vg_index_merge: source %d has no fp32 rows", s);
        total += sources[s]->n;
    }
    VG_CHECK(total < 0xFFFFFFFFll, VG_ERR_INVALID_ARG, "vg_index_merge: %lld source rows (row ids are uint32)", (long long)total);
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = vg::pick_stream(ctx, stream);
    vg::MergeStaged staged;
    vg_index *merged = nullptr;
    const int32_t status = vg::merge_run(ctx, sources, deleted, n_sources, total, staged, &merged, old_to_new, new_source, new_row, st);
    if (status != VG_OK) {
        (void)hipStreamSynchronize(st);
        (void)vg_index_destroy(merged);
        return status;
    }
    *out = merged;
    return VG_OK;
}
