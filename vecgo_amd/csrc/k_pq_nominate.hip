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

// The nomination from the codes (vg_index_enable_pq_nomination_from_codes) takes more than 128 queries — the persistent
// tile's batches; the gathered fill has no 128-row form — and has its own crossover against the scan (tools/pq_nominate_codes_time.py,
// ms scanned / from the codes, k = 10 and k = 100): 129 queries x 100k rows 0.31 / 0.24 and 0.53 / 0.32, x 300k 0.71 / 0.31, x 1M
// 2.0 / 0.56; 1024 x 1M 12.5 / 1.68, 1024 x 10M 118 / 14.8 — it won at every batch measured, the smallest 12.9M pairs.
constexpr int64_t kPqNomCodesMinPairs = 13000000;

// whether a batch takes the nomination (device queries; ascending table sums over the whole segment, no row filter)
bool pq_nomination_applies(const vg_index *idx, const float *d_queries, int64_t nq, int k, const uint8_t *mask, bool desc)
{
    const int mode = idx->pq_nom.mode();
    const int64_t min_pairs = mode == 2 ? kPqNomCodesMinPairs : kPqNomMinPairs;
    return mode && !mask && !desc && (mode == 1 || nq > 128) && (nq * idx->n >= min_pairs || hook(kHookPqNomAlways)) && k <= kNomMaxK &&
           idx->n > k && idx->pq->k == 256 && aligned16(d_queries);
}

// nominated_pass with the PQ re-score.  (From the codes the GEMM's operands are the image's, bit for bit: the same margin,
// pq_nominate_eps, holds.)
int32_t pq_nominated_pass(vg_index *idx, const float *q, int64_t nq, int k, uint32_t *oid, float *osc, hipStream_t st, std::vector<int> &failed)
{
    const vg_pq *pq = idx->pq;
    // per pass: the queries' tables (BuildDistanceTable, the reference's layout), then the table sums of the nominees
    return nominated_pass(idx, idx->pq_nom, false, q, nq, k, nullptr, 0, static_cast<size_t>(pq->m) * 256, oid, osc, st, failed,
                          [&](const float *qq, int64_t cnt, const ProbeNominated &nom, float *tables, uint32_t *pid, float *psc, int *fail) -> int32_t {
                              VG_TRY(launch_pq_build_table(pq, qq, cnt, tables, false, st));
                              return launch_nominated_verify<false>(PqTableRow{idx->d_pq_rows, tables, pq->m, pq->subdim, idx->dim}, qq,
                                                                    idx->pq_nom.norm_max, cnt, nom, k, pid, psc, fail, st);
                          });
}
}  // namespace vg

// vg_index_enable_pq_nomination (mode 1) and vg_index_enable_pq_nomination_from_codes (mode 2); fn: the entry point's name.
// Turning a mode off, or on again, drops that mode only; turning it on drops the other one too, but only once nothing can refuse.
static int32_t pq_nomination_enable(vg_index *idx, int mode, int32_t on, void *stream, const char *fn)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
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
    return vg::nom_build(idx->pq_nom, idx->n, idx->dim, vg::NomImage::body_bytes(idx->n, dim_pad, from_codes), from_codes, st,
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
                         });
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
    if (mode) *mode = idx->pq_nom.mode();
    if (held_bytes) *held_bytes = idx->pq_nom.held_bytes(idx->n);
    return VG_OK;
}
