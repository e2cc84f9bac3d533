// k_prefilter.hip — the engine's bitmap strategy for selective filters (internal/engine/search.go:500-737): score only the
// rows a filter keeps.
//
//   vg_mask_to_rows           FilterResult.ToArrayInto (search.go:617-627) for a batch of masks: the ids of the set bits,
//                             ascending, one list per query.
//   vg_search_flat_prefilter  the loop of search.go:602-736 over one resident segment: the listed rows are fetched by id, scored
//                             with distance.SquaredL2 / distance.Dot and the best k kept in one CandidateHeap.
//
// Compaction keeps row order, so it is a scan: a workgroup owns a tile of kCompactTile rows of one mask (a thread one 32-bit
// word of it); (1) every tile counts its set bits, (2) one workgroup per mask turns the tile counts into offsets and the
// mask's total, (3) every tile writes its ids behind its offset.  A single mask over 1M rows is 123 tiles: the chip is covered
// whatever the batch.  Masks sit at any byte address: 32-bit loads where address and stride allow, bytes otherwise.
//
// The search: the totals are read back (the call's one wait) and size the lists exactly; the lists of a chunk of queries form
// one CSR block, a shared mask one list; the score kernel writes one key (make_key) per (query, listed row) — per query
// `longest` slots, the longest list of the chunk — and launch_thr_select_lists (k_flat_threshold.hip) takes the best k of every
// key list.  A list is cut into chunks of kScoreChunk rows, one workgroup each: a long list is spread over the chip, a short one
// costs one workgroup (the grid is (chunks of the longest list, queries): a workgroup past its own list's end returns at once).
// One mask for the batch: a workgroup also owns a group of the queries; each of its 16-lane groups stages ONE listed row in
// LDS and scores it against every query of the group, so a row is gathered once per query group, not once per query.
// Queries whose scores may hold a NaN are replayed through the CandidateHeap (vg_cand_replay.hpp) with the engine's
// Pop-then-Push at capacity (CandHeapPopPushPolicy).
#include <algorithm>
#include <vector>

#include "vg_cand_replay.hpp"
#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_internal.hpp"
#include "vg_scan.hpp"
#include "vg_search.hpp"

namespace vg {
namespace {

constexpr int kCompactTile = VG_MASK_ROWS_TILE_ROWS;  // rows of one workgroup of the compaction: a 32-bit mask word per thread
constexpr int kCompactThreads = kScanThreads;  // (block_scan and prefix_kernel, vg_scan.hpp)
static_assert(kCompactTile == kCompactThreads * 32, "a thread keeps one 32-bit word of the tile");
constexpr int kScoreChunk = VG_PREFILTER_CHUNK_ROWS;  // listed rows of one workgroup of the score kernels
constexpr int kScoreThreads = 256;
constexpr int kScoreGroups = kScoreThreads / 16;      // (query, row) pairs in flight per workgroup; rows a workgroup stages
constexpr int kScoreLdsMax = 128 * 1024;              // the staged rows' LDS: longer rows are staged fewer at a time
static_assert(kScoreChunk % kScoreGroups == 0, "a chunk is whole passes of the workgroup's 16-lane groups");

// the mask bits of rows byte0 * 8 .. byte0 * 8 + 31, those at or above `rows` cleared
__device__ __forceinline__ uint32_t mask_word32(const uint8_t *__restrict__ m, int64_t byte0, int64_t nbytes, int64_t rows, int words)
{
    uint32_t w = 0;
    if (byte0 + 4 <= nbytes && words) {
        w = *reinterpret_cast<const uint32_t *>(m + byte0);
    } else {
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (byte0 + b < nbytes) w |= static_cast<uint32_t>(m[byte0 + b]) << (8 * b);
    }
    const int64_t left = rows - byte0 * 8;
    if (left < 32) w &= left > 0 ? (1u << left) - 1u : 0u;
    return w;
}

// (1) tile_cnt[list * tiles + tile] <- the set bits of the tile; one workgroup per (list, tile)
__global__ __launch_bounds__(kCompactThreads) void mask_tile_count_kernel(const uint8_t *__restrict__ mask, int64_t mask_stride, int64_t rows,
                                                                          int64_t tiles, int words, uint32_t *__restrict__ tile_cnt)
{
    __shared__ int wsum[kCompactThreads / 64];
    const int64_t list = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int64_t byte0 = tile * (kCompactTile / 8) + threadIdx.x * 4;
    int c = __popc(mask_word32(mask + list * mask_stride, byte0, (rows + 7) >> 3, rows, words));
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = static_cast<uint32_t>(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

// (2) one workgroup per mask turns its tile counts into offsets and the mask's total: prefix_kernel (vg_scan.hpp)

// (3) the tile's ids, ascending, behind its offset.  List l goes to out + l * out_stride, at most out_stride ids of it
// (list_off null), or — the search's CSR block — to out + list_off[l] - list_off[0], whole.
__global__ __launch_bounds__(kCompactThreads) void mask_scatter_kernel(const uint8_t *__restrict__ mask, int64_t mask_stride, int64_t rows,
                                                                       int64_t tiles, int words, const uint32_t *__restrict__ tile_off,
                                                                       uint32_t *__restrict__ out, int64_t out_stride,
                                                                       const int64_t *__restrict__ list_off)
{
    __shared__ long long wsum[kCompactThreads / 64];
    const int64_t list = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int64_t byte0 = tile * (kCompactTile / 8) + threadIdx.x * 4;
    uint32_t w = mask_word32(mask + list * mask_stride, byte0, (rows + 7) >> 3, rows, words);
    const int c = __popc(w);
    long long total;
    const long long inc = block_scan(c, wsum, total);
    if (total == 0) return;
    uint32_t *dst = list_off ? out + (list_off[list] - list_off[0]) : out + list * out_stride;
    const int64_t cap = list_off ? (int64_t(1) << 62) : out_stride;
    int64_t at = static_cast<int64_t>(tile_off[blockIdx.x]) + inc - c;
    const uint32_t row0 = static_cast<uint32_t>(byte0 * 8);
    while (w && at < cap) {
        dst[at++] = row0 + static_cast<uint32_t>(__builtin_ctz(w));
        w &= w - 1;
    }
}

inline int mask_words32(const uint8_t *p, int64_t stride) { return ((reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(stride)) & 3) == 0 ? 1 : 0; }

// steps 1 and 2 for `lists` masks: tile_off[lists * tiles] <- each tile's offset in its list, tot64 / tot32[lists] (null: not
// wanted) <- the lists' lengths
int32_t launch_mask_count(const uint8_t *mask, int64_t mask_stride, int64_t lists, int64_t rows, uint32_t *tile_off, int64_t *tot64, int *tot32,
                          hipStream_t st)
{
    const int64_t tiles = (rows + kCompactTile - 1) / kCompactTile;
    VG_LAUNCH(mask_tile_count_kernel, dim3(static_cast<unsigned>(lists * tiles)), dim3(kCompactThreads), 0, st, mask, mask_stride, rows, tiles,
              mask_words32(mask, mask_stride), tile_off);
    VG_LAUNCH(prefix_kernel<uint32_t>, dim3(static_cast<unsigned>(lists)), dim3(kCompactThreads), 0, st, tile_off, tiles, tot64, tot32);
    return VG_OK;
}

int32_t launch_mask_scatter(const uint8_t *mask, int64_t mask_stride, int64_t lists, int64_t rows, const uint32_t *tile_off, uint32_t *out,
                            int64_t out_stride, const int64_t *list_off, hipStream_t st)
{
    const int64_t tiles = (rows + kCompactTile - 1) / kCompactTile;
    VG_LAUNCH(mask_scatter_kernel, dim3(static_cast<unsigned>(lists * tiles)), dim3(kCompactThreads), 0, st, mask, mask_stride, rows, tiles,
              mask_words32(mask, mask_stride), tile_off, out, out_stride, list_off);
    return VG_OK;
}

// what both entry points refuse about a batch of masks' size (one workgroup per (mask, tile), ids are uint32)
int32_t mask_lists_check(const char *fn, int64_t lists, int64_t rows)
{
    VG_CHECK(rows < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "%s: %lld rows, fewer than 2^31 are supported", fn, (long long)rows);
    const int64_t tiles = (rows + kCompactTile - 1) / kCompactTile;
    VG_CHECK(lists < (int64_t(1) << 31) && lists * tiles < (int64_t(1) << 31), VG_ERR_UNSUPPORTED,
             "%s: %lld masks of %lld tiles, fewer than 2^31 tiles per call are supported", fn, (long long)lists, (long long)tiles);
    return VG_OK;
}

// ---- the score kernels: one key per (query, listed row) ---------------------------------------------------------------
// Query q of the chunk (blockIdx.y) owns the list at rows + list_off[q] - list_off[0] of counts[q] ids; its keys go to
// keys + q * key_cap in list order.  One 16-lane group per pair, distance.SquaredL2 / Dot in the reference's order.
template <bool DOT>
__global__ __launch_bounds__(kScoreThreads) void prefilter_score_kernel(const float *__restrict__ base, int dim, const float *__restrict__ queries,
                                                                        const uint32_t *__restrict__ rows, const int64_t *__restrict__ list_off,
                                                                        const int *__restrict__ counts, uint64_t *__restrict__ keys,
                                                                        int64_t key_cap)
{
    const int64_t q = blockIdx.y;
    const int64_t c = counts[q], r0 = static_cast<int64_t>(blockIdx.x) * kScoreChunk;
    if (r0 >= c) return;
    const int m = static_cast<int>(c - r0 < kScoreChunk ? c - r0 : kScoreChunk);
    const Sub16 sub = Sub16::make(threadIdx.x);
    const float *qv = queries + q * dim;
    const uint32_t *lst = rows + (list_off ? list_off[q] - list_off[0] : 0) + r0;  // (null: one list for every query)
    uint64_t *out = keys + q * key_cap + r0;
    for (int i = threadIdx.x >> 4; i < m; i += kScoreGroups) {
        const uint32_t id = lst[i];
        const float v = exact_pair16<DOT, kPair>(base + static_cast<int64_t>(id) * dim, qv, dim, sub);
        if ((threadIdx.x & 15) == 0) out[i] = make_key(v, id, DOT);
    }
}

// One list (`count` ids at rows) for every query.  Workgroup (blockIdx.x, blockIdx.y) owns a chunk of the list and queries
// blockIdx.y * q_per ..; `staged` (<= kScoreGroups) of its 16-lane groups keep one listed row each in LDS (dim_pad floats, a
// whole number of float4: every staged row is 16-byte aligned whatever dim is) and score it against each of the queries.  A
// group reads only the row it staged itself: no workgroup barrier.
template <bool DOT>
__global__ __launch_bounds__(kScoreThreads) void prefilter_score_shared_kernel(const float *__restrict__ base, int dim, int dim_pad, int vec4,
                                                                               const float *__restrict__ queries, int64_t nq, int q_per,
                                                                               const uint32_t *__restrict__ rows, int64_t count, int staged,
                                                                               uint64_t *__restrict__ keys, int64_t key_cap)
{
    extern __shared__ float4 prefilter_lds[];
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kScoreChunk;
    if (r0 >= count) return;
    const int m = static_cast<int>(count - r0 < kScoreChunk ? count - r0 : kScoreChunk);
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    if (g >= staged) return;  // (whole 16-lane groups; nothing below is a workgroup barrier)
    const Sub16 sub = Sub16::make(threadIdx.x);
    const int64_t qa = static_cast<int64_t>(blockIdx.y) * q_per, qb = qa + q_per < nq ? qa + q_per : nq;
    float *mine = reinterpret_cast<float *>(prefilter_lds) + static_cast<size_t>(g) * dim_pad;
    for (int i = g; i < m; i += staged) {
        const uint32_t id = rows[r0 + i];
        const float *src = base + static_cast<int64_t>(id) * dim;
        __threadfence_block();  // the previous row's reads are behind us (a wave's LDS accesses complete in order; this keeps the compiler's order)
        if (vec4) {
            for (int j = l; j < (dim >> 2); j += 16) reinterpret_cast<float4 *>(mine)[j] = reinterpret_cast<const float4 *>(src)[j];
        } else {
            for (int j = l; j < dim; j += 16) mine[j] = src[j];
        }
        __threadfence_block();
        for (int64_t q = qa; q < qb; q++) {
            const float v = exact_pair16<DOT, kPair>(mine, queries + q * dim, dim, sub);
            if (l == 0) keys[q * key_cap + r0 + i] = make_key(v, id, DOT);
        }
    }
}

// the rows one workgroup can stage: up to one per 16-lane group, fewer for rows beyond 8 KiB, 0: a row does not fit
inline int score_staged_rows(int dim)
{
    const int64_t row_bytes = static_cast<int64_t>((dim + 3) & ~3) * 4;
    return static_cast<int>(std::min<int64_t>(kScoreGroups, kScoreLdsMax / std::max<int64_t>(row_bytes, 16)));
}

// a chunk of the call's queries: [q0, q1), the longest of their lists and the lists' sum
struct QueryChunk {
    int64_t q0, q1, longest, total;
};

}  // namespace
}  // namespace vg

VG_API int32_t vg_mask_to_rows(vg_ctx *ctx, const uint8_t *mask, int64_t mask_stride, int64_t nq, int64_t rows, uint32_t *out_rows,
                               int64_t out_stride, int64_t *counts, void *stream)
{
    VG_CHECK(ctx, VG_ERR_INVALID_ARG, "vg_mask_to_rows: NULL context");
    VG_CHECK(nq >= 0 && rows >= 0 && out_stride >= 0, VG_ERR_INVALID_ARG, "vg_mask_to_rows: nq = %lld, rows = %lld, out_stride = %lld: negative",
             (long long)nq, (long long)rows, (long long)out_stride);
    if (nq == 0) return VG_OK;
    VG_TRY(vg::mask_lists_check("vg_mask_to_rows", nq, rows));
    const int64_t nbytes = (rows + 7) / 8;
    VG_CHECK(mask || nbytes == 0, VG_ERR_INVALID_ARG, "vg_mask_to_rows: NULL mask");
    VG_CHECK(out_rows || out_stride == 0, VG_ERR_INVALID_ARG, "vg_mask_to_rows: out_stride = %lld but out_rows is NULL", (long long)out_stride);
    VG_CHECK(mask_stride >= nbytes || (mask_stride == 0 && nq <= 1), VG_ERR_INVALID_ARG,
             "vg_mask_to_rows: mask_stride = %lld, a query's mask has %lld bytes (0 only for a single query)", (long long)mask_stride,
             (long long)nbytes);
    if (out_stride == 0 && !counts) return VG_OK;
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = vg::pick_stream(ctx, stream);
    const size_t slots = static_cast<size_t>(nq) * static_cast<size_t>(out_stride);
    vg::DevOut<uint32_t> out;
    VG_TRY(out.init(out_rows, slots, st, vg::kAnyAlign));
    vg::DevOut<int64_t> cnt;
    VG_TRY(cnt.init(counts, static_cast<size_t>(nq), st, vg::kAnyAlign));
    if (slots > 0) VG_HIP(hipMemsetAsync(out.ptr, 0xFF, slots * sizeof(uint32_t), st));  // VG_INVALID_ID behind every list
    bool host_mask = false;
    if (rows == 0) {
        if (counts) VG_HIP(hipMemsetAsync(cnt.ptr, 0, static_cast<size_t>(nq) * sizeof(int64_t), st));
    } else {
        host_mask = !vg::is_device_ptr(mask);
        vg::DevIn<uint8_t> mk;
        VG_TRY(mk.init(mask, vg::mask_span(mask, mask_stride, nq, rows), st, vg::kAnyAlign));
        const int64_t tiles = (rows + vg::kCompactTile - 1) / vg::kCompactTile;
        vg::DevTmp<uint32_t> tile_off;
        VG_TRY(tile_off.init(static_cast<size_t>(nq * tiles), st));
        vg::ProfScope prof(ctx, "mask_to_rows", st);
        VG_TRY(vg::launch_mask_count(mk.ptr, mask_stride, nq, rows, tile_off.ptr, cnt.ptr, nullptr, st));
        if (out_stride > 0) VG_TRY(vg::launch_mask_scatter(mk.ptr, mask_stride, nq, rows, tile_off.ptr, out.ptr, out_stride, nullptr, st));
    }
    VG_TRY(out.finish());
    VG_TRY(cnt.finish());
    if (host_mask) VG_HIP(hipStreamSynchronize(st));  // the caller's mask has been read
    return VG_OK;
}

VG_API int32_t vg_search_flat_prefilter(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask, int64_t mask_stride,
                                        uint32_t *ids, float *scores, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_search_flat_prefilter: NULL index");
    VG_CHECK(nq >= 0 && k >= 0, VG_ERR_INVALID_ARG, "vg_search_flat_prefilter: negative nq or k");
    VG_CHECK(k <= vg::kThrMaxResults, VG_ERR_UNSUPPORTED, "vg_search_flat_prefilter: k=%d exceeds %d", k, vg::kThrMaxResults);
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(queries && ids && scores, VG_ERR_INVALID_ARG, "vg_search_flat_prefilter: NULL buffer");
    VG_CHECK(mask, VG_ERR_INVALID_ARG, "vg_search_flat_prefilter: NULL mask (a search without a filter is vg_search_flat)");
    const int64_t n = idx->n, nbytes = (n + 7) / 8;
    VG_CHECK(nq <= 1 || mask_stride == 0 || mask_stride >= nbytes, VG_ERR_INVALID_ARG,
             "vg_search_flat_prefilter: mask_stride %lld is shorter than a mask (%lld bytes)", (long long)mask_stride, (long long)nbytes);
    VG_CHECK(n == 0 || idx->d_vectors, VG_ERR_NOT_READY, "vg_search_flat_prefilter: index has no fp32 vectors");
    const bool shared = mask_stride == 0 && nq > 1;  // one list, every row of it scored against the whole batch
    const int64_t lists = (mask_stride == 0) ? 1 : nq;
    VG_TRY(vg::mask_lists_check("vg_search_flat_prefilter", lists, n));

    vg::SearchIO io;
    VG_TRY(io.init(idx->ctx, stream, queries, static_cast<size_t>(nq) * idx->dim, ids, scores, static_cast<size_t>(nq) * k));
    hipStream_t st = io.st;
    vg_ctx *ctx = idx->ctx;
    const bool dot = idx->metric != VG_METRIC_L2;
    const int dim = idx->dim;
    if (n == 0) {  // no row: the selection over empty lists pads
        vg::DevTmp<int> zero, kept;
        vg::DevTmp<uint64_t> none;
        VG_TRY(zero.init(static_cast<size_t>(nq), st));
        VG_TRY(kept.init(static_cast<size_t>(nq), st));
        VG_TRY(none.init(1, st));
        VG_HIP(hipMemsetAsync(zero.ptr, 0, sizeof(int) * static_cast<size_t>(nq), st));
        VG_TRY(vg::launch_thr_select_lists(dot, none.ptr, 1, zero.ptr, nullptr, nq, 1, k, io.oid.ptr, io.osc.ptr, kept.ptr, st));
        return io.finish();
    }
    vg::DevIn<uint8_t> mk;  // (the kernels below read a mask at any byte address)
    VG_TRY(mk.init(mask, vg::mask_span(mask, mask_stride, nq, n), st, vg::kAnyAlign));

    // 1. count: every tile's offset in its list, the lists' lengths and their offsets in one CSR block; the lengths come back
    const int64_t tiles = (n + vg::kCompactTile - 1) / vg::kCompactTile;
    vg::DevTmp<uint32_t> tile_off;
    vg::DevTmp<int64_t> cnt64, list_off;
    vg::DevTmp<int> cnt32;
    VG_TRY(tile_off.init(static_cast<size_t>(lists * tiles), st));
    VG_TRY(cnt64.init(static_cast<size_t>(lists), st));
    VG_TRY(list_off.init(static_cast<size_t>(lists), st));
    VG_TRY(cnt32.init(static_cast<size_t>(nq), st));
    std::vector<int64_t> h_cnt(static_cast<size_t>(lists));
    {
        vg::ProfScope prof(ctx, "prefilter_count", st);
        VG_TRY(vg::launch_mask_count(mk.ptr, mask_stride, lists, n, tile_off.ptr, cnt64.ptr, cnt32.ptr, st));
        VG_HIP(hipMemcpyAsync(list_off.ptr, cnt64.ptr, sizeof(int64_t) * static_cast<size_t>(lists), hipMemcpyDeviceToDevice, st));
        VG_LAUNCH(vg::prefix_kernel<int64_t>, dim3(1), dim3(vg::kCompactThreads), 0, st, list_off.ptr, lists, nullptr, nullptr);
    }
    VG_HIP(hipMemcpyAsync(h_cnt.data(), cnt64.ptr, sizeof(int64_t) * static_cast<size_t>(lists), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));

    // query chunks whose lists (4 bytes per id) and keys (8 bytes per query and slot of the chunk's longest list) stay inside the
    // context's scratch cap; a query whose own list exceeds it is a chunk of its own
    const int64_t cap_bytes = vg::hook(vg::kHookPrefilterSmallScratch) ? 65536 : vg::scratch_cap(ctx);  // (the hook: several chunks for a test batch)
    std::vector<vg::QueryChunk> chunks;
    if (shared) {
        const int64_t len = h_cnt[0], slot = std::max<int64_t>(len, 1);
        const int64_t qc = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 65535), (cap_bytes - len * 4) / (slot * 8)));
        for (int64_t q0 = 0; q0 < nq; q0 += qc) chunks.push_back({q0, std::min(nq, q0 + qc), len, len});
    } else {
        vg::QueryChunk c{0, 0, 0, 0};
        for (int64_t q = 0; q < nq; q++) {
            int64_t longest = std::max(c.longest, h_cnt[q]), total = c.total + h_cnt[q];
            if (q > c.q0 && (total * 4 + (q - c.q0 + 1) * std::max<int64_t>(longest, 1) * 8 > cap_bytes || q - c.q0 >= 65535)) {
                chunks.push_back(c);  // query q opens the next chunk
                c = vg::QueryChunk{q, q, 0, 0};
                longest = total = h_cnt[q];
            }
            c.q1 = q + 1;
            c.longest = longest;
            c.total = total;
        }
        chunks.push_back(c);
    }
    size_t rows_bytes = 4, keys_bytes = 8, cnt_max = 1;
    for (const vg::QueryChunk &c : chunks) {
        rows_bytes = std::max(rows_bytes, static_cast<size_t>(c.total) * sizeof(uint32_t));
        keys_bytes = std::max(keys_bytes, static_cast<size_t>(c.q1 - c.q0) * static_cast<size_t>(std::max<int64_t>(c.longest, 1)) * sizeof(uint64_t));
        cnt_max = std::max(cnt_max, static_cast<size_t>(c.q1 - c.q0));
    }
    vg::ArenaCall ar(ctx, st);
    const int i_rows = ar.add(rows_bytes), i_keys = ar.add(keys_bytes), i_ocnt = ar.add(sizeof(int32_t) * cnt_max);
    VG_TRY(ar.commit());
    uint32_t *rows = ar.get<uint32_t>(i_rows);
    uint64_t *keys = ar.get<uint64_t>(i_keys);
    int32_t *ocnt = ar.get<int32_t>(i_ocnt);
    if (shared) {  // the one list's length, per query slot of the selection
        VG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cnt32.ptr), static_cast<int>(h_cnt[0]), static_cast<size_t>(nq), st));
    }

    const int staged = vg::score_staged_rows(dim);
    const int dim_pad = (dim + 3) & ~3;
    const int vec4 = dim % 4 == 0 && vg::aligned16(idx->d_vectors) ? 1 : 0;
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        const vg::QueryChunk &c = chunks[ci];
        const int64_t cnt = c.q1 - c.q0, key_cap = std::max<int64_t>(c.longest, 1);
        const float *qp = io.q.ptr + c.q0 * dim;
        if (c.total > 0) {
            // 2. compact: the chunk's lists as one CSR block (a shared mask: its list, once)
            if (!shared || ci == 0) {
                vg::ProfScope prof(ctx, "prefilter_compact", st);
                const int64_t l0 = shared ? 0 : c.q0;
                VG_TRY(vg::launch_mask_scatter(mk.ptr + l0 * mask_stride, mask_stride, shared ? 1 : cnt, n, tile_off.ptr + l0 * tiles, rows, 0,
                                               list_off.ptr + l0, st));
            }
            // 3. score
            vg::ProfScope prof(ctx, "prefilter_score", st);
            const unsigned gx = static_cast<unsigned>((c.longest + vg::kScoreChunk - 1) / vg::kScoreChunk);
            if (shared && staged > 0) {
                // about four workgroups per compute unit: the list's chunks times as many query groups as that takes
                const int64_t want = 4 * static_cast<int64_t>(std::max(ctx->compute_units, 1));
                const int64_t groups = std::max<int64_t>(1, std::min<int64_t>(cnt, (want + gx - 1) / gx));
                const int q_per = static_cast<int>((cnt + groups - 1) / groups);
                const size_t lds = static_cast<size_t>(staged) * dim_pad * sizeof(float);
                VG_TRY(vg::with_metric(dot, [&](auto dot_c) -> int32_t {
                    auto kern = vg::prefilter_score_shared_kernel<decltype(dot_c)::value>;
                    if (lds > 65536)
                        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, vg::kScoreLdsMax));
                    VG_LAUNCH(kern, dim3(gx, static_cast<unsigned>((cnt + q_per - 1) / q_per)), dim3(vg::kScoreThreads), lds, st, idx->d_vectors, dim,
                              dim_pad, vec4, qp, cnt, q_per, rows, c.longest, staged, keys, key_cap);
                    return VG_OK;
                }));
            } else {
                // (a shared list whose rows are too long to stage: every query reads it where it lies; list_off: all zero then)
                VG_TRY(vg::with_metric(dot, [&](auto dot_c) -> int32_t {
                    VG_LAUNCH(vg::prefilter_score_kernel<decltype(dot_c)::value>, dim3(gx, static_cast<unsigned>(cnt)), dim3(vg::kScoreThreads), 0, st,
                              idx->d_vectors, dim, qp, rows, shared ? nullptr : list_off.ptr + c.q0, cnt32.ptr + c.q0, keys, key_cap);
                    return VG_OK;
                }));
            }
        }
        // 4. select: the best k of every key list, padded
        vg::ProfScope prof(ctx, "prefilter_select", st);
        VG_TRY(vg::launch_thr_select_lists(dot, keys, key_cap, cnt32.ptr + c.q0, nullptr, cnt, key_cap, k, io.oid.ptr + c.q0 * k,
                                           io.osc.ptr + c.q0 * k, ocnt, st));
    }
    // 5. queries whose scores may hold a NaN: the engine's heap over the mask's rows in ascending order (search.go:717-733)
    VG_TRY(vg::launch_cand_replay<vg::CandHeapPopPushPolicy>(vg::FlatF32Scorer{idx->d_vectors, idx->d_norm_max + 1, dim, dot, 0}, io.q.ptr, dim, n, nq,
                                                             k, dot, mk.ptr, mask_stride, io.oid.ptr, io.osc.ptr, st));
    VG_TRY(io.finish());
    if (!vg::is_device_ptr(mask)) VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}
