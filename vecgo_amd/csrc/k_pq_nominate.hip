// k_pq_nominate.hip — the PQ batch search through a bfloat16 nomination (vg_index_enable_pq_nomination, _from_codes) for gfx950:
// the kernels that build the nomination's state from the codes, the verify pair's Row, which batches take it, and the pass the
// search driver (k_adc.hip) runs for them.
#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_nominate.hpp"
#include "vg_search.hpp"

// One table scan per query runs at the LDS gather rate: 12.5 ms for 1024 queries x 1M x m = 96.  A row's table sum IS a squared
// distance — sum_j |q_j - C_j[code_j]|^2 = |q - x^|^2 for the DECODED row x^ (pq.go:185-229; the table entries are computed from
// the same fp32 centroid values, pq.go:468-491) — so with the opt-in image (x^ rounded to bfloat16, 2 bytes per dimension) the batch
// runs the shared nomination (vg_nominate.hpp), re-scores with the reference's own arithmetic — BuildDistanceTable +
// pqAdcLookupAvx512 on the CODES (PqTableRow) — and proves the result (bfloat16 rounding of both operands, fp32 accumulation on
// both sides).  A query whose proof fails is scanned as before.
namespace vg {
// the batches the nomination takes: 1M x 768, m = 96, k = 10: 16 queries 0.24 ms scanned / 0.39 nominated, 32: 0.46 / 0.41, 64: 0.86 /
// 0.43, 1024: 12.4 / 1.7 (tools/pq_nominate_time.py) — the scan costs ~12 us per query and 1M rows, the nomination ~0.4 ms up to
// 128 queries; 100k rows: 128 queries 0.27 / 0.31, 256: 0.50 / 0.28 — from 24M (query, row) pairs up.  Test hook VG_PQ_NOM_ALWAYS:
// every batch.
constexpr int64_t kPqNomMinPairs = 24000000;

// one wave per row: lane l decodes sub-quantizers l, l + 64, ... — v = float32(int8) * scale ; v = v + offset, the two rounded
// operations of the reference's dequantisation (pq.go:204-214) — rounds to bfloat16 (nearest even), writes the image row
// (dim_pad elements, zeros from dim on) and the row's norm
// (ROWS false: the norms alone — pq_norms_kernel, the nomination from the codes: the same operations in the same order)
template <bool ROWS>
__device__ __forceinline__ void pq_decode_row(const uint8_t *__restrict__ codes, int64_t n, int m, int k, int sd,
                                              const int8_t *__restrict__ codebooks, const float *__restrict__ scales,
                                              const float *__restrict__ offsets, uint16_t *__restrict__ out, int dim_pad,
                                              float *__restrict__ norms, int *__restrict__ norm_max_bits)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= n) return;  // (whole waves)
    uint16_t *dst = ROWS ? out + row * dim_pad : nullptr;
    float nrm = 0.0f;
    for (int j = lane; j < m; j += 64) {
        const int c = codes[row * m + j];
        const int8_t *cb = codebooks + (static_cast<int64_t>(j) * k + c) * sd;
        const float sc = scales[j], of = offsets[j];
        for (int d = 0; d < sd; d++) {
            float v = static_cast<float>(cb[d]) * sc;
            v = v + of;
            nrm = __builtin_fmaf(v, v, nrm);
            const uint32_t b = __float_as_uint(v);
            if constexpr (ROWS) dst[j * sd + d] = static_cast<uint16_t>((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
        }
    }
    if constexpr (ROWS)
        for (int j = m * sd + lane; j < dim_pad; j += 64) dst[j] = 0;
    for (int off = 32; off > 0; off >>= 1) nrm += __shfl_xor(nrm, off);
    if (lane == 0) {
        norms[row] = nrm;
        // a NaN norm (a NaN scale / offset) must reach norm_max: NaN -> +Inf, the proof's comparisons then fail and the scan answers
        const int nb = __float_as_int(nrm == nrm ? nrm : INFINITY);  // non-negative floats order like their bits
        if (nb > *reinterpret_cast<volatile int *>(norm_max_bits)) atomicMax(norm_max_bits, nb);  // (a wave per row: only where it raises the value)
    }
}
__global__ __launch_bounds__(256) void pq_decode_bf16_kernel(const uint8_t *__restrict__ codes, int64_t n, int m, int k, int sd,
                                                             const int8_t *__restrict__ codebooks, const float *__restrict__ scales,
                                                             const float *__restrict__ offsets, uint16_t *__restrict__ out, int dim_pad,
                                                             float *__restrict__ norms, int *__restrict__ norm_max_bits)
{
    pq_decode_row<true>(codes, n, m, k, sd, codebooks, scales, offsets, out, dim_pad, norms, norm_max_bits);
}
__global__ __launch_bounds__(256) void pq_norms_kernel(const uint8_t *__restrict__ codes, int64_t n, int m, int k, int sd,
                                                       const int8_t *__restrict__ codebooks, const float *__restrict__ scales,
                                                       const float *__restrict__ offsets, float *__restrict__ norms, int *__restrict__ norm_max_bits)
{
    pq_decode_row<false>(codes, n, m, k, sd, codebooks, scales, offsets, nullptr, 0, norms, norm_max_bits);
}
// The decoded codebook of the nomination from the codes (NomImage::rows with from_codes; K = 256, sub-dimension 8): thread per entry (j, c) of
// `blocks` sub-quantizers, its 8 values decoded and rounded as pq_decode_row rounds them — 16 bytes, what the image of the decoded
// rows holds at granule j of every row with code c there; the blocks from m on are zeros, the image's padding
__global__ void pq_codebook_bf16_kernel(const int8_t *__restrict__ codebooks, const float *__restrict__ scales, const float *__restrict__ offsets,
                                        int m, int blocks, uint4 *__restrict__ cb16)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= blocks * 256) return;
    const int j = t >> 8;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (j < m) {
        const int8_t *cb = codebooks + static_cast<int64_t>(t) * 8;
        const float sc = scales[j], of = offsets[j];
#pragma unroll
        for (int d = 0; d < 8; d++) {
            float v = static_cast<float>(cb[d]) * sc;
            v = v + of;
            const uint32_t b = __float_as_uint(v);
            w[d >> 1] |= ((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16) << (16 * (d & 1));
        }
    }
    cb16[t] = make_uint4(w[0], w[1], w[2], w[3]);
}

// pqAdcLookupAvx512 (internal/simd/src/floats_avx512.c:135-167) of one row's code against a query's table in the reference's
// own layout (m rows of 256): 16 lane sums over the full groups, the _mm512_reduce_add_ps tree, the tail added in order — what
// pq_adc_scan_kernel computes from its LDS image
__device__ __forceinline__ float pq_adc_row_score(const float *__restrict__ lut, const uint8_t *__restrict__ code, int m)
{
    float s[16];
#pragma unroll
    for (int l = 0; l < 16; l++) s[l] = 0.0f;
    int i = 0;
    for (; i + 16 <= m; i += 16) {
        float t[16];
#pragma unroll
        for (int l = 0; l < 16; l++) t[l] = lut[(i + l) * 256 + code[i + l]];
#pragma unroll
        for (int l = 0; l < 16; l++) s[l] = s[l] + t[l];
    }
    float total = reduce16_regs(s);
    for (; i < m; i++) total = total + lut[i * 256 + code[i]];
    return total;
}

// the proof's margin: |s~ + |q|^2 - table sum| for any row.  bfloat16 rounding of q and x^: (2^-7 + 2^-16)(|q|^2 + |x^|^2); the GEMM's
// fp32 accumulation and the norm's: 2 dim u of the same; the table's entries ((sd + 2) u each, relative) and their 16-lane sum
// ((m / 16 + 4 + 15) u): 2 (m + sd + 6) u of the same (|q - x^|^2 <= 2 (|q|^2 + |x^|^2)).
__device__ __forceinline__ float pq_nominate_eps(int dim, int m, int sd, float qn, float norm_max)
{
    return ((4.0f * static_cast<float>(dim) + 2.0f * static_cast<float>(m + sd + 6)) * 5.9604645e-8f + 0.0078125f * 1.02f) * (qn + norm_max) + 1e-30f;
}

// the verify pair's Row (vg_nominate.hpp): the table sum of a nominated row from the codes against query q's table
struct PqTableRow {
    const uint8_t *codes;  // n * m, row-major
    const float *tables;   // per query: m rows of 256
    int m, sd, dim;        // dim = m * sd
    __device__ float score(int64_t q, const float *, uint32_t id) const
    {
        return pq_adc_row_score(tables + q * m * 256, codes + static_cast<int64_t>(id) * m, m);
    }
    __device__ float eps(float qn, float norm_max) const { return pq_nominate_eps(dim, m, sd, qn, norm_max); }
    static constexpr bool kShifted = false;  // (the GEMM multiplies the decoded rows themselves)
};

// The nomination from the codes (vg_index_enable_pq_nomination_from_codes) takes more than 128 queries on the persistent tile —
// its gathered fill has no 128-row form; fewer run the tile below when it is enabled — and has its own crossover against the scan (tools/pq_nominate_codes_time.py,
// ms scanned / from the codes, k = 10 and k = 100): 129 queries x 100k rows 0.31 / 0.24 and 0.53 / 0.32, x 300k 0.71 / 0.31, x 1M
// 2.0 / 0.56; 1024 x 1M 12.5 / 1.68, 1024 x 10M 118 / 14.8 — it won at every batch measured, the smallest 12.9M pairs.
constexpr int64_t kPqNomCodesMinPairs = 13000000;
// The same for batches of 5 .. 128 queries when the mode was enabled with on = 2 (NomImage::pq_small; reported as mode 3): the tile
// of one query tile (flat_gemm_pq_small_kernel, vg_pq_small_gemm.hpp), where a block of 32 queries' image of a row fits that
// tile's LDS (pq_small_tile_fits: m <= 318) and the codes are at least the 16 bytes of one load, from kPqNomCodesSmallMinPairs
// pairs up.
// Measured (MI355X, tools/pq_nominate_codes_time.py 10000000 small, dim 768, m = 96, k = 10, ms per call, scan / mode 3 / image
// mode, alternating windows of ~300 ms in one run on one index per segment size, every shape warmed, the median of 5; the windows
// of a leg lay within 1 % of each other, 9 % at 128 x 100k; bits equal at every shape; profiles/pq_nominate_codes_time_small.txt):
//   100k rows —   8 queries 0.040 / 0.168 / 0.208,  32: 0.077 / 0.175 / 0.277,  64: 0.134 / 0.195 / 0.346,  96: 0.189 / 0.212 / 0.338,
//                128: 0.245 / 0.244 / 0.383
//   1M rows   —   8: 0.128 / 0.340 / 0.386,  32: 0.417 / 0.347 / 0.411,  64: 0.811 / 0.363 / 0.442,  96: 1.206 / 0.387 / 0.474,
//                128: 1.601 / 0.558 / 0.509  (k = 100: 1.858 / 0.646 / 0.626)
//   10M rows  —   8: 0.970 / 2.026 / 2.445,  32: 3.734 / 2.072 / 2.552,  64: 7.418 / 2.110 / 2.594,  96: 11.12 / 2.203 / 3.099,
//                128: 14.82 / 4.009 / 3.391
// The GEMM's own time (its profile scope): 100k — 0.032, 0.037, 0.050, 0.062, 0.092 ms; 1M — 0.184, 0.189, 0.200, 0.220, 0.388
// (k = 100: 0.413); 10M — 1.730, 1.757, 1.763, 1.807, 3.571: one pass costs the same from 8 to 96 queries, 128 queries are two
// passes (two launches of two blocks).  What bounds a pass is NOT established.  It is not HBM (96 MB of code bytes a pass over 1M
// rows: 0.012 ms at 8 TB/s; 0.55 TB/s reached) and not the matrix unit (49 GFLOP at one block: 0.02 ms).  A pass gathers 1.5 GB of
// codebook entries through the vector caches: 8.3 TB/s at 1M rows, 8.7 TB/s at 10M — over 256 CUs at 2.4 GHz that is 13.5 .. 14.2 B
// a clock and CU, 21 .. 22 % of the 64 B a clock a CU's vector cache nominally delivers (39 TB/s over the chip; the nominal figure
// was not measured here).  At a fifth of that rate the gather's throughput is not shown to be the limit: with 18 loads in flight a
// wave and 2 .. 3 waves a SIMD the pass may as well be bound by the gathers' latency or by occupancy; no counter run separated
// them.  The rest of a call (0.16 ms: the sample, the pick, the tables and the verify) is not this kernel's.  From the ISA
// (re-read after the change below): the K loop's waits are all counted, vmcnt(17) and vmcnt(16) before a step's two matrix
// instructions — the 16 gathers and the code load issued behind the slot — and the ring's registers are reused in place (no copy
// at a chunk's end, unlike both siblings); a gather is three vector instructions (shift, and-or, shift), not two.  The epilogue's
// first wait is vmcnt(19), for the tile's two norms, loaded ahead of the tile's first chunk: the next position's 16 gathers and 2
// code loads stay in flight under it (the chunk loop is a do-while: with a path around it the compiler had put vmcnt(1) there,
// a drain at every tile's end).  What still drains the ring: an APPEND — the returning atomic is waited for with vmcnt(0), in the
// branch only a lane with a row below its threshold takes — and the first steps of a tile wait two loads deeper than the ring
// asks, the norms' loads lying between two chunks' gathers.  Gathers run a chunk of 128 dimensions ahead and the codes two.  The
// timings above were taken before that change of the tile's end.  A second run after it (the same file, run 2) gave every mode-3
// figure within 3 % of the table, 96 x 10M 2.321 ms (5 % above): the change bought nothing measurable, the crossover is the same.
// The nomination LOST to the scan at every 100k-row shape (0.24x .. 0.89x, a tie at 128 x 100k) and at 8 queries at every size
// (0.38x at 1M, 0.48x at 10M: a pass over the codes costs the same for 8 queries as for 96, the scan 12 us a query and 1M rows).
// It won from 32 queries x 1M rows up: 1.20x, 64: 2.23x, 96: 3.12x, 128: 2.87x; 10M rows: 1.80x, 3.52x, 5.05x, 3.70x — by far more
// than the spread.  Because 8 x 10M (80M pairs) lost where 32 x 1M (32M pairs) won, a product alone does not separate them: the
// batch size 8 stays on the scan as a whole (kPqNomCodesSmallMinQueries: 32, the smallest batch measured that won; nothing between
// 8 and 32 queries was measured) and the constant is the smallest product measured at which the nomination won, 32 x 1M; nothing
// between 12.8M and 32M pairs was measured.  Against the image mode it is 0.71x .. 0.85x of the time up to 96 queries and 1.10x ..
// 1.18x at 128 (two passes), holding 4 bytes a row where the image holds 16x the codes.  Test hook VG_PQ_NOM_ALWAYS: any batch of
// 5 queries up.
constexpr int kPqNomCodesSmallMinQueries = 32;
constexpr int64_t kPqNomCodesSmallMinPairs = 32000000;

// The same for FILTERED batches from the codes (on & 4, NomImage::pq_masked): above 128 queries the big tile with the filter in its
// epilogue, 5 .. 128 queries the small tile's MASKED variants (on & 3 == 2).  A filter makes the scan a little cheaper and the
// nomination mostly dearer, so these stand apart from the constants above.
// Measured (MI355X, tools/pq_nominate_codes_time.py 1000000 filtered, dim 768, m = 96, k = 10, ms per call, filtered scan / filtered
// nomination, alternating windows of ~100 ms in one run on one index, the windows of a leg within 1 % of each other (4 % at 32 x
// 100k); profiles/pq_nominate_codes_time_filtered.txt), a batch filter keeping 100 % / 10 % / 1 % of the rows, then one per query
// keeping 10 %; bits equal and no query rescanned in any line.
// Above 128 queries (the big tile): 129 x 100k, 10 %: 0.282 / 0.304 — LOST, it keeps the scan; 129 x 1M, 10 % and 1 %: 2.087 / 0.644,
// 1.979 / 0.815; 256 x 1M, 1 %: 3.173 / 0.860; 1024 x 1M: 13.49 / 1.868, 13.46 / 2.244, 12.61 / 2.756, 15.88 / 2.682 (k = 100, 10 %:
// 27.07 / 2.755).  The scan gets 7 % faster at 1 % kept, the big tile 48 % slower (its GEMM 1.575 -> 2.444 ms: thresholds from a
// hundredth of the sample pass more rows, and every pass reads a filter bit), as for INT4.  The constant is the smallest measured
// product that won, 129 x 1M; nothing between 12.9M and 129M pairs was measured.
// 5 .. 128 queries (the small tile), 100k rows: 32 queries 0.084 / 0.179, 0.078 / 0.184, 0.073 / 0.181, 0.079 / 0.188; 128: 0.264 /
// 0.261, 0.241 / 0.274, 0.223 / 0.303, 0.244 / 0.323 — lost everywhere but for a tie under the keep-all filter: 100k rows keep the
// scan.  1M rows: 8 queries 0.141 / 0.348, 0.136 / 0.341, 0.126 / 0.271, 0.140 / 0.347 — lost 0.40x .. 0.46x, so the floor of 32
// queries stays for filtered batches; 32: 0.472 / 0.356, 0.472 / 0.350, 0.420 / 0.281, 0.511 / 0.360; 128: 1.723 / 0.565, 1.703 /
// 0.565, 1.604 / 0.464, 1.943 / 0.732 — won 1.33x .. 3.46x.  The constant is the smallest measured product that won, 32 x 1M, with
// nothing between 12.8M and 32M pairs measured: as unfiltered.
// What the slice skip buys (the GEMM's scope, 1M rows, 100 % / 10 % / 1 % kept): 32 queries 0.191 / 0.190 / 0.127 ms, 8 queries
// 0.183 / 0.182 / 0.118, 128 queries (two launches) 0.385 / 0.389 / 0.292: at 1 % kept 53 % of the 64-row slices are empty and a
// pass costs 34 % less (its gathers are the pass's cost, see above); at 10 % one slice in 850 is empty and nothing changes.  One
// filter per query has no skip and reads a bit for every score under its threshold: 0.197 at 32 queries, 0.542 at 128.  Over 100k
// rows (391 tiles for 512 workgroups and more: a workgroup has one tile, a skipped slice shortens nothing) the 1 % filter makes the
// pass dearer, 0.095 -> 0.141 ms at 128 queries, by the appends its looser thresholds let through.
constexpr int64_t kPqNomCodesMaskedMinPairs = 129000000;
constexpr int kPqNomCodesMaskedSmallMinQueries = 32;
constexpr int64_t kPqNomCodesMaskedSmallMinPairs = 32000000;

// whether a batch takes the nomination (device queries; ascending table sums over the whole segment; mask: the batch's row filter,
// per query or one for all, or null — a filtered batch only from the codes, where the mode was enabled with on & 4)
bool pq_nomination_applies(const vg_index *idx, const float *d_queries, int64_t nq, int k, const uint8_t *mask, bool desc)
{
    const int mode = idx->pq_nom.mode();
    if (mask && !(mode == 2 && idx->pq_nom.pq_masked)) return false;
    const bool small = mode == 2 && nq <= 128;  // the small tile's batches, where it was enabled and takes the rows
    if (small && (!idx->pq_nom.pq_small || nq < 5 || !pq_small_tile_takes(idx->pq->m, idx->n))) return false;
    if (small && nq < (mask ? kPqNomCodesMaskedSmallMinQueries : kPqNomCodesSmallMinQueries) && !hook(kHookPqNomAlways)) return false;
    const int64_t min_pairs = small       ? (mask ? kPqNomCodesMaskedSmallMinPairs : kPqNomCodesSmallMinPairs)
                              : mode == 2 ? (mask ? kPqNomCodesMaskedMinPairs : kPqNomCodesMinPairs)
                                          : kPqNomMinPairs;
    return mode && !desc && (nq * idx->n >= min_pairs || hook(kHookPqNomAlways)) && k <= kNomMaxK && idx->n > k && idx->pq->k == 256 &&
           aligned16(d_queries);
}

// nominated_pass with the PQ re-score.  (From the codes the GEMM's operands are the image's, bit for bit: the same margin,
// pq_nominate_eps, holds.  A row filter changes none of it: the bound is per (query, row), and a filter only takes rows away, from
// the list and from the rows outside it alike.)
int32_t pq_nominated_pass(vg_index *idx, const float *q, int64_t nq, int k, const uint8_t *mask, int64_t mask_stride, uint32_t *oid, float *osc,
                          hipStream_t st, std::vector<int> &failed)
{
    const vg_pq *pq = idx->pq;
    // per pass: the queries' tables (BuildDistanceTable, the reference's layout), then the table sums of the nominees
    return nominated_pass(idx, idx->pq_nom, false, q, nq, k, mask, mask_stride, static_cast<size_t>(pq->m) * 256, oid, osc, st, failed,
                          [&](const float *qq, int64_t cnt, const ProbeNominated &nom, float *tables, uint32_t *pid, float *psc, int *fail) -> int32_t {
                              VG_TRY(launch_pq_build_table(pq, qq, cnt, tables, false, st));
                              return launch_nominated_verify<false>(PqTableRow{idx->d_pq_rows, tables, pq->m, pq->subdim, idx->dim}, qq,
                                                                    idx->pq_nom.norm_max, cnt, nom, k, pid, psc, fail, st);
                          });
}
}  // namespace vg

// vg_index_enable_pq_nomination (mode 1) and vg_index_enable_pq_nomination_from_codes (mode 2; `on` as bits: on & 3 == 2: small batches too,
// on & 4: filtered batches too — of a mode, so 4 alone is none); fn: the entry point's name.
// Turning a mode off, or on again, drops that mode only; turning it on drops the other one too, but only once nothing can refuse.
static int32_t pq_nomination_enable(vg_index *idx, int mode, int32_t on, void *stream, const char *fn)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(mode != 2 || (on != 4 && on <= 6), VG_ERR_INVALID_ARG, "%s: on=%d is a flag without a mode, or above 6", fn, on);
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    if (idx->pq_nom.mode() == mode) VG_TRY(vg::nom_free(idx->pq_nom, st));
    if (!on) return VG_OK;
    VG_CHECK(idx->pq && idx->d_pq_rows, VG_ERR_NOT_READY, "%s: index has no PQ codes", fn);
    const vg_pq *pq = idx->pq;
    VG_CHECK(pq->trained, VG_ERR_NOT_TRAINED, "ProductQuantizer not trained");
    VG_CHECK(pq->k == 256, VG_ERR_UNSUPPORTED, "%s: needs numCentroids == 256 (got %d), as the table scan does", fn, pq->k);
    const bool from_codes = mode == 2;
    VG_CHECK(!from_codes || pq->subdim == 8, VG_ERR_UNSUPPORTED,
             "%s: needs sub-vectors of 8 dimensions (got %d): a 16-byte granule of a row is one centroid", fn, pq->subdim);
    VG_TRY(vg::nom_free(idx->pq_nom, st));
    const int dim_pad = vg::nom_dim_pad(idx->dim), blocks = dim_pad / 8;
    VG_TRY(vg::nom_build(idx->pq_nom, idx->n, idx->dim, vg::NomImage::body_bytes(idx->n, dim_pad, from_codes), from_codes, st,
                         [&](const vg::NomImage &b, int *norm_max_bits) {
                             const dim3 rows_grid(static_cast<unsigned>((idx->n + 3) / 4));
                             if (!from_codes) {
                                 hipLaunchKernelGGL(vg::pq_decode_bf16_kernel, rows_grid, dim3(256), 0, st, idx->d_pq_rows, idx->n, pq->m, pq->k, pq->subdim,
                                                    pq->d_codebooks, pq->d_scales, pq->d_offsets, b.rows, b.dim_pad, b.norms, norm_max_bits);
                                 return;
                             }
                             hipLaunchKernelGGL(vg::pq_codebook_bf16_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, pq->d_codebooks,
                                                pq->d_scales, pq->d_offsets, pq->m, blocks, reinterpret_cast<uint4 *>(b.rows));
                             hipLaunchKernelGGL(vg::pq_norms_kernel, rows_grid, dim3(256), 0, st, idx->d_pq_rows, idx->n, pq->m, pq->k, pq->subdim,
                                                pq->d_codebooks, pq->d_scales, pq->d_offsets, b.norms, norm_max_bits);
                         }));
    idx->pq_nom.pq_small = from_codes && on > 0 && (on & 3) == 2;  // (1, 3 and a negative value are 1)
    idx->pq_nom.pq_masked = from_codes && on > 0 && (on & 4) != 0;
    return VG_OK;
}

VG_API int32_t vg_index_enable_pq_nomination(vg_index *idx, int32_t on, void *stream)
{
    return pq_nomination_enable(idx, 1, on, stream, "vg_index_enable_pq_nomination");
}

VG_API int32_t vg_index_enable_pq_nomination_from_codes(vg_index *idx, int32_t on, void *stream)
{
    return pq_nomination_enable(idx, 2, on, stream, "vg_index_enable_pq_nomination_from_codes");
}

VG_API int32_t vg_index_pq_nomination_info(const vg_index *idx, int32_t *mode, int64_t *held_bytes)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_pq_nomination_info: NULL index");
    // (3: from the codes, small batches too; 6 and 7: 2 and 3 with filtered batches)
    if (mode) *mode = (idx->pq_nom.pq_small ? 3 : idx->pq_nom.mode()) | (idx->pq_nom.pq_masked ? 4 : 0);
    if (held_bytes) *held_bytes = idx->pq_nom.held_bytes(idx->n);
    return VG_OK;
}
