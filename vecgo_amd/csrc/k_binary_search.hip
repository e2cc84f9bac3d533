// k_binary_search.hip — vg_search_binary: the exhaustive Hamming top-k over an index's binary codes (vg_index_set_binary_codes).
// BinaryQuantizer's codes (internal/quantization/binary.go:86-154: bit i = v[i] >= threshold, ceil(dim/64) uint64 words a row)
// are the densest the library holds; the reference scores them one pair at a time (ComputeHammingDistance, :158-171 — encode the
// query, popcount(xor)).  The scan over every row is this library's: the screen in front of vg_rerank at 1 bit a dimension.
//
// The score of a pair is an integer in [0, dim], so a key is exact and final as the kernel computes it: the high word is the
// ordered bit pattern of float(h) (make_key; float(h) is exact below 2^24 and its pattern rises strictly with h), the low word the
// row — (Score, RowID) under one unsigned compare, the key every merge of the library reads.  Whether a row may enter a list is
// decided on the integer h; a key is built only for a row that passes.  No score can be a NaN: there is no replay.
//
// binary_search_kernel<QB>: a workgroup of 4 waves carries a block of QB queries over its slice of 64-row tiles.
//   rows     A wave takes a tile's bytes as they lie in memory — rows are row-major, so a tile is 64 * code_bytes contiguous bytes
//            — with one 16-byte load per lane and trip (coalesced: a lane-per-row read of 96-byte rows would touch 64 cache lines
//            per load), and writes the two 8-byte halves to its own LDS stage at [row][word], rows an odd number of words apart
//            (no bank conflict when a lane then reads its own row's words, 8 bytes at a time).  Codes longer than 128 bytes
//            (dim > 1024) go through the stage in pieces of 128 bytes a row, so that the stage stays 8.5 KiB a wave at any dim; a
//            piece is 64 runs of 128 contiguous bytes.  The 16-byte loads need rows of whole 16-byte chunks or a one-piece tile;
//            what is left — dim > 1024 with an odd number of words — loads 8 bytes per lane instead: the same results, slower.
//   queries  The block's codes are encoded once per call (binary_encode_kernel) and lie in LDS as [word][query]: a word's QB
//            values are read at a wave-uniform address (broadcast) and feed QB xor + bit-count-and-add pairs per row word.
//   select   Per query a WaveTopK and the integer h of its k-th key; wg_rank_merge, the paged driver and launch_topk_merge
//            (vg_search.hpp) as in every scan.  A batch mask's tile without a kept row is not read.
// QB: 16 for batches of 5 or more, 4 up to 4 queries, 1 for one query.  What bounds it is not registers — 16 accumulators, 16
// key lists (32 registers) and the staged words: 112 VGPRs at QB = 16, no scratch, 4 waves a SIMD as the 36 KiB of static LDS
// allow anyway (profiles/kernel_resources.txt) — but the
// last block of a batch, whose missing queries are computed and dropped, and the LDS the query block takes (code_bytes * QB, at
// most 24 KiB beside the 36 KiB of stage and merge lists: QB = 16 up to dim 12288, 4 up to 49152, 1 up to 196608).
#include <algorithm>
#include <climits>
#include <vector>

#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_nominate.hpp"
#include "vg_scan_slices.hpp"
#include "vg_search.hpp"

namespace vg {

constexpr int kBsWaves = 4;      // waves (64-row tiles in flight) of a workgroup
constexpr int kBsPiece = 16;     // 8-byte words of a row in the stage at once
constexpr int kBsSmallGrid = 2;  // workgroups / slices under the test hook VG_BINARY_SMALL_GRID
constexpr size_t kBsMaxQueryLds = 24 * 1024;

template <int QB>
__global__ __launch_bounds__(kBsWaves * 64) void binary_search_kernel(const uint64_t *__restrict__ qcodes, const uint64_t *__restrict__ codes,
                                                                      int64_t n, int64_t n_tiles, int tile_stride, int words, const uint8_t *__restrict__ mask,
                                                                      int64_t mask_stride, int slices, int nq, int k,
                                                                      uint64_t *__restrict__ partial, const uint64_t *__restrict__ min_keys)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t bs_q[];  // the block's query codes, [words][QB]
    __shared__ __attribute__((aligned(16))) uint64_t stage_all[kBsWaves][64 * (kBsPiece + 1)];
    __shared__ uint64_t lists[kBsWaves * 64];
    __shared__ int valid[kBsWaves];
    const int ng = (nq + QB - 1) / QB;
    const int b = blockIdx.x;
    int qg, s;
    if ((slices & 7) == 0) {  // the query blocks of one slice on one XCD: they share the slice in its L2
        const int xcd = b & 7, o = b >> 3;
        qg = o % ng;
        s = (o / ng) * 8 + xcd;
    } else {  // (the test hook's 2 slices)
        qg = b % ng;
        s = b / ng;
    }
    const int q0 = qg * QB;
    const int cnt = nq - q0 < QB ? nq - q0 : QB;
    const int64_t t0 = n_tiles * s / slices, t1 = n_tiles * (s + 1) / slices;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < words * QB; e += kBsWaves * 64) {  // a block's missing queries repeat its last one and are not merged
        const int w = e / QB, qi = e - w * QB;
        bs_q[e] = qcodes[static_cast<int64_t>(q0 + (qi < cnt ? qi : cnt - 1)) * words + w];
    }
    __syncthreads();
    WaveTopK tk[QB];
    int tau_h[QB];  // h of the k-th key (every h until k keys were seen)
#pragma unroll
    for (int qi = 0; qi < QB; qi++) {
        tk[qi].init(k);
        tau_h[qi] = INT_MAX;
    }
    const bool batch_mask = mask != nullptr && mask_stride == 0;
    uint64_t *stage = stage_all[wave];
    const int pieces = (words + kBsPiece - 1) / kBsPiece;
    const bool wide = pieces == 1 || (words & 1) == 0;  // a 16-byte chunk lies in one row, or the tile is one run of bytes
    for (int64_t ti = t0 + wave; ti < t1; ti += kBsWaves) {
        const int64_t tile = ti * tile_stride;  // (the nomination's threshold sample: every tile_stride-th tile)
        const int64_t row = tile * 64 + lane;
        const bool inb = row < n;
        const bool keep = inb && (!batch_mask || mask_bit(mask, row));  // a batch filter's bit: read once for the QB queries
        if (batch_mask && !__ballot(keep)) continue;                    // (uniform) not read
        const uint64_t *tbase = codes + tile * 64 * words;              // (the index pads its codes to whole tiles)
        int acc[QB];
#pragma unroll
        for (int qi = 0; qi < QB; qi++) acc[qi] = 0;
        for (int p = 0; p < pieces; p++) {
            const int len = words - p * kBsPiece < kBsPiece ? words - p * kBsPiece : kBsPiece;
            const int stride = len | 1;
            const uint32_t inv = (65536u + len - 1) / len;  // u / len == (u * inv) >> 16 for u < 1024, len <= 16
            const uint64_t *pbase = tbase + p * kBsPiece;
            if (wide) {
                for (int u = 2 * lane; u < 64 * len; u += 128) {
                    const int r0 = static_cast<int>((static_cast<uint32_t>(u) * inv) >> 16), o0 = u - r0 * len;
                    const uint4 *src = reinterpret_cast<const uint4 *>(pbase + r0 * words + o0);
                    const uint4 v = QB == 1 ? load_stream(src) : *src;  // a batch's next query block reads the codes again
                    const bool wrap = o0 + 1 == len;  // (one piece, an odd number of words: the second half is the next row's)
                    stage[r0 * stride + o0] = (static_cast<uint64_t>(v.y) << 32) | v.x;
                    stage[wrap ? (r0 + 1) * stride : r0 * stride + o0 + 1] = (static_cast<uint64_t>(v.w) << 32) | v.z;
                }
            } else {
                for (int u = lane; u < 64 * len; u += 64) {
                    const int r0 = static_cast<int>((static_cast<uint32_t>(u) * inv) >> 16), o0 = u - r0 * len;
                    stage[r0 * stride + o0] = pbase[r0 * words + o0];
                }
            }
            // the lanes read what other lanes of the wave wrote: order the stage's writes, reads and next writes
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint64_t *mine = stage + lane * stride;
            const uint64_t *qw = bs_q + p * kBsPiece * QB;
            for (int w = 0; w < len; w++) {
                const uint64_t x = mine[w];
#pragma unroll
                // (uniform address: a broadcast read.  The compiler counts each word into a fresh register and adds: 5 instructions
                // per word and query)
                for (int qi = 0; qi < QB; qi++) acc[qi] += __popcll(x ^ qw[w * QB + qi]);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int qi = 0; qi < QB; qi++) {
            if (qi < cnt) {
                const bool live = batch_mask ? keep : inb && mask_bit(mask ? mask + (q0 + qi) * mask_stride : nullptr, row);
                if (__ballot(live && acc[qi] <= tau_h[qi])) {
                    uint64_t key = live ? make_key(static_cast<float>(acc[qi]), static_cast<uint32_t>(row), false) : kKeyMax;
                    if (min_keys && key <= min_keys[q0 + qi]) key = kKeyMax;
                    tk[qi].offer(key, lane);
                    tau_h[qi] = tk[qi].tau == kKeyMax ? INT_MAX : static_cast<int>(key_score(tk[qi].tau, false));
                }
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < QB; qi++) {
        if (qi < cnt) {
            wg_rank_merge<kBsWaves>(tk[qi], lists, valid, wave, lane, tid, k, partial + (static_cast<int64_t>(q0 + qi) * slices + s) * k);
            __syncthreads();
        }
    }
}

// the scan of nq queries (device buffers): their codes, the launch shape, pages beyond 64 results, the merge
// the launch of one scan over `tiles` tiles, every tile_stride-th of the index's: `slices` lists of kk keys per query in `partial`
static int32_t launch_binary_scan(const vg_index *idx, const uint64_t *qcodes, int64_t nq, int qb, int64_t tiles, int tile_stride,
                                  const uint8_t *mask, int64_t mask_stride, int slices, int kk, uint64_t *partial, const uint64_t *floor,
                                  const char *scope, hipStream_t st)
{
    const int words = (idx->dim + 63) / 64;
    const size_t cb = static_cast<size_t>(words) * 8;
    const int64_t max_q = (1ll << 30) / slices * qb;  // whole query blocks per launch
    for (int64_t q0 = 0; q0 < nq; q0 += max_q) {
        const int64_t cnt = std::min<int64_t>(nq - q0, max_q);
        const dim3 grid(static_cast<unsigned>((cnt + qb - 1) / qb * slices)), block(kBsWaves * 64);
        const uint64_t *qc = qcodes + q0 * words;
        const uint64_t *rows = reinterpret_cast<const uint64_t *>(idx->d_bin_rows);
        const uint8_t *mm = mask ? mask + q0 * mask_stride : nullptr;
        uint64_t *pp = partial + q0 * slices * kk;
        const uint64_t *ff = floor ? floor + q0 : nullptr;
        ProfScope prof(idx->ctx, scope, st);
        if (qb == 16)
            VG_LAUNCH(binary_search_kernel<16>, grid, block, cb * 16, st, qc, rows, idx->n, tiles, tile_stride, words, mm, mask_stride, slices,
                      static_cast<int>(cnt), kk, pp, ff);
        else if (qb == 4)
            VG_LAUNCH(binary_search_kernel<4>, grid, block, cb * 4, st, qc, rows, idx->n, tiles, tile_stride, words, mm, mask_stride, slices,
                      static_cast<int>(cnt), kk, pp, ff);
        else
            VG_LAUNCH(binary_search_kernel<1>, grid, block, cb, st, qc, rows, idx->n, tiles, tile_stride, words, mm, mask_stride, slices,
                      static_cast<int>(cnt), kk, pp, ff);
    }
    return VG_OK;
}

// the nomination's threshold sample (k_binary_nominate.hip): every 64th tile scored by the scan kernel, the sel_k best per query
static int64_t binary_sample_tiles(const vg_index *idx) { return ((idx->n + 63) / 64 + 63) / 64; }
int binary_sample_slices(const vg_index *idx, int64_t cnt)
{
    return scan_slices((cnt + 15) / 16, (binary_sample_tiles(idx) + kBsWaves - 1) / kBsWaves, idx->ctx->compute_units, 4);
}
int32_t launch_binary_sample(const vg_index *idx, const uint64_t *qcodes, int64_t cnt, int sel_k, int slices, uint64_t *partial, uint32_t *ids,
                             float *thr, hipStream_t st)
{
    VG_TRY(launch_binary_scan(idx, qcodes, cnt, 16, binary_sample_tiles(idx), 64, nullptr, 0, slices, sel_k, partial, nullptr,
                              "binary_nom_sample", st));
    return launch_topk_merge(partial, cnt, slices, sel_k, false, ids, thr, st);
}

int32_t binary_scan_batch(vg_index *idx, const float *q, int64_t nq, int k, const uint8_t *mask, int64_t mask_stride, uint32_t *oid,
                                 float *osc, hipStream_t st)
{
    const int dim = idx->dim, cus = idx->ctx->compute_units;
    const int64_t n = idx->n, n_tiles = (n + 63) / 64;
    const int words = (dim + 63) / 64;
    const size_t cb = static_cast<size_t>(words) * 8;
    int qb = nq >= 5 ? 16 : nq > 1 ? 4 : 1;
    while (qb > 1 && cb * qb > kBsMaxQueryLds) qb /= 4;
    VG_CHECK(cb * qb <= kBsMaxQueryLds, VG_ERR_UNSUPPORTED, "vg_search_binary: dim %d exceeds %d", dim, static_cast<int>(kBsMaxQueryLds) * 8);
    const int slices = hook(kHookBinarySmallGrid) ? kBsSmallGrid : scan_slices((nq + qb - 1) / qb, (n_tiles + kBsWaves - 1) / kBsWaves, cus, 4);
    ArenaCall ar(idx->ctx, st);
    PagedTopK pages;  // a wave keeps 64 keys: k > 64 comes in pages of 64, one scan per page
    pages.add(ar, nq, k, slices);
    const int i_qc = ar.add(static_cast<size_t>(nq) * cb);
    VG_TRY(ar.commit());
    uint64_t *qcodes = ar.get<uint64_t>(i_qc);
    VG_TRY(launch_binary_encode(q, nq, dim, idx->bin_threshold, reinterpret_cast<uint8_t *>(qcodes), st));
    return pages.run(ar, slices, false, oid, osc, st, [&](int kk, uint64_t *partial, const uint64_t *floor) -> int32_t {
        return launch_binary_scan(idx, qcodes, nq, qb, n_tiles, 1, mask, mask_stride, slices, kk, partial, floor, "binary_search", st);
    });
}

}  // namespace vg

// Binary codes of an index: n * vg_binary_code_bytes(dim) bytes row-major, what vg_binary_encode writes.  Held once, in that
// layout, padded with zero rows to whole 64-row tiles (the scan reads a tile's bytes as one run); NULL drops them.
VG_API int32_t vg_index_set_binary_codes(vg_index *idx, float threshold, const uint8_t *codes, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_set_binary_codes: NULL index");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    if (idx->d_bin_rows) {
        VG_HIP(hipStreamSynchronize(st));
        VG_HIP(hipFree(idx->d_bin_rows));
        idx->d_bin_rows = nullptr;
    }
    idx->bin_bytes = idx->bin_nominated = idx->bin_rescanned = 0;
    if (!codes || idx->n == 0) return VG_OK;
    idx->bin_threshold = threshold;
    const size_t cb = static_cast<size_t>(vg_binary_code_bytes(idx->dim));
    const size_t used = static_cast<size_t>(idx->n) * cb, bytes = static_cast<size_t>((idx->n + 63) / 64) * 64 * cb;
    uint8_t *rows = nullptr;
    VG_HIP(hipMalloc(reinterpret_cast<void **>(&rows), bytes));
    hipError_t e = bytes > used ? hipMemsetAsync(rows + used, 0, bytes - used, st) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(rows, codes, used, hipMemcpyDefault, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {  // nothing half-filled stays on the index
        (void)hipFree(rows);
        VG_HIP(e);
    }
    idx->d_bin_rows = rows;
    idx->bin_bytes = static_cast<int64_t>(bytes);
    return VG_OK;
}

VG_API int32_t vg_index_binary_info(const vg_index *idx, int64_t *code_bytes, int64_t *nominated, int64_t *rescanned)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_binary_info: NULL index");
    if (code_bytes) *code_bytes = idx->bin_bytes;
    if (nominated) *nominated = idx->bin_nominated;
    if (rescanned) *rescanned = idx->bin_rescanned;
    return VG_OK;
}

VG_API int32_t vg_search_binary(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask, int64_t mask_stride,
                                uint32_t *ids, float *scores, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_search_binary: NULL index");
    VG_CHECK(nq >= 0 && k >= 0, VG_ERR_INVALID_ARG, "vg_search_binary: negative nq or k");
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(idx->n == 0 || idx->d_bin_rows, VG_ERR_NOT_READY, "vg_search_binary: index has no binary codes");
    VG_CHECK(queries && ids && scores, VG_ERR_INVALID_ARG, "vg_search_binary: NULL buffer");
    VG_CHECK(k <= 512, VG_ERR_UNSUPPORTED, "vg_search_binary: k=%d exceeds 512", k);
    if (nq > 1) VG_CHECK_MASK_STRIDE("vg_search_binary", mask, mask_stride, idx->n);
    vg::SearchIO io;
    VG_TRY(io.init(idx->ctx, stream, queries, static_cast<size_t>(nq) * idx->dim, ids, scores, static_cast<size_t>(nq) * k, mask,
                   vg::mask_span(mask, nq > 1 ? mask_stride : 0, nq, idx->n)));
    if (idx->n == 0)
        VG_TRY(vg::empty_results(nq, k, false, io.oid.ptr, io.osc.ptr, io.st));
    else if (vg::binary_nomination_applies(idx, nq, k, io.mk.ptr)) {
        // the matrix cores (k_binary_nominate.hip); the scan for the queries whose list overflowed or came up short
        std::vector<int> failed;
        VG_TRY(vg::binary_nominated_pass(idx, io.q.ptr, nq, k, io.oid.ptr, io.osc.ptr, io.st, failed));
        VG_TRY(vg::rescan_failed(failed, io.q.ptr, idx->dim, k, nullptr, 0, 0, io.oid.ptr, io.osc.ptr, io.st,
                                 [&](const float *fq, int64_t nf, const uint8_t *, int64_t, uint32_t *fid, float *fsc) {
                                     return vg::binary_scan_batch(idx, fq, nf, k, nullptr, 0, fid, fsc, io.st);
                                 }));
    } else
        VG_TRY(vg::binary_scan_batch(idx, io.q.ptr, nq, k, io.mk.ptr, nq > 1 ? mask_stride : 0, io.oid.ptr, io.osc.ptr, io.st));
    return io.finish();
}
