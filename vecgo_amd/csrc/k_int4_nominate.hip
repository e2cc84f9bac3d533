// k_int4_nominate.hip — the INT4 batch search through a bfloat16 nomination (vg_index_enable_int4_nomination) for gfx950: the
// kernels that build the nomination's state from the nibble codes, the verify pair's Row, which batches take it, and the pass the
// search driver (vg_search_int4, k_int4_search.hip) runs for them.
#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_nominate.hpp"
#include "vg_search.hpp"

// The multi-query scan (int4_search_mq_kernel) decodes every code once per 8 queries and is bound by the vector ALU: 55.3 ms per
// 1024 queries x 1M x 768.  The reference decodes x^_d = fl(fl(fl(c_d / 15) diff_d) + min_d) (int4_table_kernel, k_int4.hip; int4.go:
// 152-163).  With c'_d = c_d - 8, an integer in -8 .. 7 that bfloat16 holds exactly, the scale s_d = fl(diff_d / 15), y = c' o s and
// mid_d = fl(min_d + 8 s_d):  q.x^ ~ (q o s).c' + q.mid.  The GEMM multiplies the query image bf16(fl(q_d s_d)) — the ONLY rounded
// operand — by the exact c', converted from the row-major codes inside the tile's fill (flat_gemm_int4_big_kernel, vg_flat_gemm.hpp)
// and, for the sampled tiles, in the call's scratch (int4_sample_rows_kernel, k_flat.hip): both score
//     s' = |x^|^2 - 2 (q o s).c',
// the exact L2 score's space moved by |q|^2 and by the per-query constant 2 q.mid, which the verify pair takes back (Int4Row::shift).
// vg_search_int4 scores L2 under every metric: there is no Dot form.  (Why c - 8 and not 2 c - 15: vg_flat_gemm.hpp, kBigInt4.)
// The state (NomImage, from_codes with `int4`): rows = mid as dim_pad floats, the scale as dim_pad floats (zeros from dim on, both),
// then one float H2 = sum_d (|min_d| + |diff_d|)^2 (the margin's decode term); norms = |x^|^2 summed from the decoded values;
// norm_max = max over the rows of max(|x^|^2, |y|^2), so that 2.002 (|q|^2 + norm_max) lies above every |s'| (flat_thr_cap_kernel)
// and B = |q|^2 + norm_max scales the margin.  NaN -> +Inf: a non-finite min or diff makes every proof fail and the scan answers.
// Held: 4 n + 8 dim_pad + 8 bytes — nothing in rows x dim.
namespace vg {
// From how many (query, row) pairs a batch takes the nomination.  Measured (MI355X, tools/int4_nominate_time.py, dim 768, ms per
// call, scan / nominated, both in one run on one index): k = 10 — 129 queries x 100k rows 1.251 / 0.238, 1024 x 100k 5.760 / 0.471,
// 1024 x 1M 55.607 / 1.802, 1024 x 10M 552.0 / 14.99; k = 100 — 1024 x 1M 112.57 / 2.387.  The nomination won at every shape: the
// constant is the smallest measured product, 129 x 100k, and nothing below it was measured.  Test hook VG_INT4_NOM_ALWAYS: any.
constexpr int64_t kInt4NomMinPairs = 12900000;
// The same for batches of 5 .. 128 queries under on = 2 (flat_gemm_int4_small_kernel).  Measured (MI355X, tools/int4_nominate_time.py
// [max_rows] small, dim 768, k = 10, ms per call, scan / nominated, alternating windows of ~300 ms in one run on one index; the windows
// of a leg lay within 1 % of each other, 3 % at one shape): 100k rows — 8 queries 0.198 / 0.173, 32 0.383 / 0.175, 64 0.592 / 0.200,
// 96 0.995 / 0.218, 128 0.956 / 0.254; 1M — 8 0.662 / 0.269, 32 2.010 / 0.279, 64 3.720 / 0.363, 96 7.344 / 0.414, 128 7.143 / 0.565
// (k = 100: 15.29 / 0.762); 10M — 8 4.788 / 1.199, 32 17.63 / 1.266, 64 34.84 / 1.921, 96 70.23 / 2.318, 128 69.21 / 3.558.  The
// nomination won at every shape, by 14 % at the smallest: the constant is the smallest measured product, 8 x 100k, and nothing below
// it was measured.  Test hook VG_INT4_NOM_ALWAYS: any.
constexpr int64_t kInt4NomSmallMinPairs = 800000;
// The same for FILTERED batches (on & 4): a filter makes the scan cheaper (a selective one by the tiles it drops), the nomination
// hardly, so these stand apart from the two above.  Measured (MI355X, tools/int4_nominate_time.py 1000000 filtered, dim 768, k = 10,
// ms per call, filtered scan / filtered nomination, alternating windows of ~100 ms in one run on one index, the windows of a leg
// within 1 % of each other; profiles/int4_nominate_time_filtered.txt), a batch filter keeping 100 % / 10 % / 1 % of the rows, then one
// per query keeping 10 %.  Above 128 queries: 129 x 100k, 10 %: 1.141 / 0.314; 1024 x 1M: 55.31 / 1.687, 55.18 / 2.076, 28.35 / 3.054,
// 56.03 / 2.547 (k = 100, 10 %: 111.5 / 2.921).  The nomination won everywhere: the smallest measured product, 129 x 100k.
// 5 .. 128 queries, 100k rows: 8 queries 0.198 / 0.179, 0.163 / 0.176, 0.140 / 0.173, 0.161 / 0.178 — the scan wins under every
// selective filter —; 32: 0.383 / 0.182, 0.306 / 0.182, 0.256 / 0.183, 0.304 / 0.190; 128: 0.954 / 0.269, 0.874 / 0.288, 0.597 / 0.308,
// 0.883 / 0.327.  1M rows: 8: 0.662 / 0.283, 0.584 / 0.280, 0.495 / 0.256, 0.587 / 0.287; 32: 2.022 / 0.290, 1.942 / 0.288, 1.357 / 0.264,
// 1.965 / 0.306; 128: 7.164 / 0.578, 7.090 / 0.583, 4.040 / 0.513, 7.199 / 0.794.  From 32 x 100k up the nomination won under every
// filter kind: that product is the constant, and 8 x 100k keeps the scan.  No query was rescanned in any line.
constexpr int64_t kInt4NomMaskedMinPairs = 12900000;
constexpr int64_t kInt4NomMaskedSmallMinPairs = 3200000;

// one workgroup of 64 lanes: mid, the scale and H2
__global__ void int4_mid_kernel(const float *__restrict__ mins, const float *__restrict__ diff, int dim, int dim_pad, float *__restrict__ mid)
{
    float h2 = 0.0f;
    for (int j = threadIdx.x; j < dim_pad; j += 64) {
        const float s = j < dim ? diff[j] / 15.0f : 0.0f;
        mid[dim_pad + j] = s;
        mid[j] = j < dim ? __builtin_fmaf(8.0f, s, mins[j]) : 0.0f;  // (8 s is exact: one rounding)
        if (j < dim) {
            const float h = fabsf(mins[j]) + fabsf(diff[j]);
            h2 = __builtin_fmaf(h, h, h2);
        }
    }
    for (int off = 32; off > 0; off >>= 1) h2 += __shfl_xor(h2, off);
    if (threadIdx.x == 0) mid[2 * dim_pad] = h2;
}
// 16 lanes per row (a wave: four rows; lane t of a row takes bytes t, t + 16, ... — any dim, any alignment): |x^|^2 from the
// reference's three rounded operations, |y|^2 beside it for norm_max.  (The sums' order is this kernel's own: they feed the GEMM's
// starting value and the margin, which counts dim roundings for them.)
__global__ __launch_bounds__(256) void int4_codes_norms_kernel(const uint8_t *__restrict__ codes, int64_t n, int dim, const float *__restrict__ mins,
                                                               const float *__restrict__ diff, float *__restrict__ norms,
                                                               int *__restrict__ norm_max_bits)
{
    const int64_t row = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 4;
    const int t = threadIdx.x & 15, row_bytes = (dim + 1) / 2;
    float nrm = 0.0f, cn = 0.0f;
    if (row < n) {
        const uint8_t *cp = codes + row * row_bytes;
        for (int b = t; b < row_bytes; b += 16) {
            const uint32_t byte = cp[b];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int j = 2 * b + e;
                if (j < dim) {
                    const uint32_t c = e ? byte & 15u : byte >> 4;
                    const float a = static_cast<float>(c) / 15.0f;
                    const float p = a * diff[j];
                    const float x = p + mins[j];
                    const float y = static_cast<float>(static_cast<int>(c) - 8) * (diff[j] / 15.0f);
                    nrm = __builtin_fmaf(x, x, nrm);
                    cn = __builtin_fmaf(y, y, cn);
                }
            }
        }
    }
    for (int off = 8; off > 0; off >>= 1) {
        nrm += __shfl_xor(nrm, off);
        cn += __shfl_xor(cn, off);
    }
    if (row < n && t == 0) norms[row] = nrm;
    // NaN -> +Inf, as the SQ8 state's kernels have it (sq8_dequant_bf16_kernel, k_sq8_scan.hip)
    float mx = 0.0f;
    if (row < n) mx = nrm == nrm && cn == cn ? fmaxf(nrm, cn) : INFINITY;
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & 63) == 0) atomicMax(norm_max_bits, __float_as_int(mx));  // non-negative floats order like their bits
}

// the verify pair's Row (vg_nominate.hpp): Int4Quantizer.L2Distance of a nominated row with the bits the scan writes
// (int4_l2_precomputed on the quantizer's table: vg_device.hpp), the score space's constant and its margin
struct Int4Row {
    const uint8_t *rows;  // n * dim / 2
    const float *table;
    int dim;
    const float *mid;  // dim_pad floats, the scale's dim_pad, then H2
    int dim_pad;
    static constexpr bool kShifted = true;
    __device__ float score(int64_t, const float *qv, uint32_t id) const
    {
        return int4_l2_precomputed(qv, rows + static_cast<int64_t>(id) * (dim >> 1), dim, table);
    }
    __device__ float shift(const float *qv, int lane) const  // the lane's share of q.mid
    {
        float c = 0.0f;
        for (int j = lane; j < dim; j += 64) c = __builtin_fmaf(qv[j], mid[j], c);
        return c;
    }
    // |s' + |q|^2 - 2 q.mid - L2Distance| for any row, u = 2^-24, B = |q|^2 + norm_max, H2 as above.  Sq8CodesRow::eps's terms
    // (k_sq8_scan.hip) with the INT4 decode in the place of SQ8's single fma:
    //  query rounding   the image is q_d s_d (1 + d)(1 + b), |d| <= u (the fp32 product), |b| <= 2^-8 (bfloat16, nearest even); the
    //                   products with c' are exact in fp32: |sum - q.y| <= (2^-8 + 2 u) |q||y| <= (2^-9 + u) B, the score twice that.
    //                   (|y|^2 <= norm_max up to the (dim + 1) u of its own sum: inside the leading term's 1.001)
    //  GEMM sum         the tile starts at (t - |x^|^2) / 2 (at most 1.501 B, by flat_thr_cap_kernel), adds dim products (S = sum
    //                   |products| <= 0.51 B) and the key's fma: screen_gemm_eps's term (k_flat.hip), 4.03 (dim + 16) u
    //  norms            the stored |x^|^2 is a sum of dim fmas in int4_codes_norms_kernel's order: dim u B
    //  the decode       x^_d = (c/15 (1 + a) diff_d (1 + b) + min_d)(1 + e) with |a|, |b|, |e| <= u — the rounding of c / 15, of its
    //                   product with diff, of the sum: two more than SQ8's fma — and y_d + mid_d = c diff_d/15 (1 + g) + min_d +
    //                   m mid_d with |g| <= u (the rounding of diff / 15 in the scale; 8 s is exact) and |m| <= u (mid's one fma):
    //                   |x^_d - y_d - mid_d| <= u (3 |c diff_d / 15| + |x^_d| + |mid_d|) + O(u^2).  No row's norm bounds these: min
    //                   and c diff / 15 may cancel in every row.  Each of the three is at most h_d = |min_d| + |diff_d| (1 + 3 u):
    //                   |q.x^ - q.(y + mid)| <= 5 u |q| sqrt(H2) <= 2.5 u (|q|^2 + H2), the score twice that; taken as 6 u for the
    //                   second-order terms
    //  q.mid            the wave's sum: dim / 64 fmas and 6 additions, (dim / 64 + 8) u |q||mid|, and |mid| <= |x^| + |y| + the
    //                   decode term <= 2 sqrt(norm_max) (1 + O(u)), |q||mid| <= B; taken twice: (dim / 32 + 16) u
    //  the comparison   tau + |q|^2 - 2 q.mid - eps: three roundings of at most 5 B, and |q|^2 as the kernel sums it,
    //                   (dim / 64 + 7) u: 16 u + (dim / 64 + 7) u
    //  the reference    int4L2DistancePrecomputedAvx512's order: q_d - x^_d rounded (2 u on its square), sixteen lane sums of dim / 16
    //                   fmas each (a 32-block feeds its two halves into the same sixteen, in order), the four-level tree over them
    //                   and the tail: (dim / 16 + 23) u |q - x^|^2 <= (dim / 8 + 46) u B
    //  2^-8 + 2 u + (4.03 (dim + 16) + dim + dim / 32 + 16 + 16 + dim / 64 + 7 + dim / 8 + 46) u  <=  2^-8 1.001 + (6 dim + 160) u,
    //  + 6 u (|q|^2 + H2).  At dim 768: 4.19e-3 B.  Denormal products the matrix unit may flush: below 1e-35 dim, inside the absolute
    // term.  tests/test_int4_nomination_bound_cpu.py models the sums.
    // A row filter (on & 4) changes none of it: the bound is per (query, row), and a filter only takes rows away — from the list
    // and from the rows outside it alike — so the same margin separates the kept rows' k-th score from the kept rows outside.
    __device__ float eps(float qn, float norm_max) const
    {
        const float d = static_cast<float>(dim), u = 5.9604645e-8f;
        return (0.00390625f * 1.001f + (6.0f * d + 160.0f) * u) * (qn + norm_max) + 6.0f * u * (qn + mid[2 * dim_pad]) + 1e-30f;
    }
};

// The nomination takes more than 128 queries — the persistent tile's batches; the register-staged fill has no 128-row form — over
// the whole segment, unfiltered, rows of whole 16-byte halves of a K step (dim % 32 == 0), from kInt4NomMinPairs pairs up.
// Enabled with on = 2 (NomImage::int4_small) it also takes 5 .. 128 queries, on the tile of one query tile
// (flat_gemm_int4_small_kernel, vg_int4_small_gemm.hpp) from kInt4NomSmallMinPairs pairs up, where a block of 32 queries' image of
// a row fits that tile's LDS (int4_small_tile_fits: dim <= 2496).  Enabled with on & 4 (NomImage::int4_masked) a batch under a row
// filter — one per query, or one for the batch — takes it too, within what on & 3 allows and from the filtered constants up.
// (device queries; mask: the batch's row filter, per query or one for all, or null)
bool int4_nomination_applies(const vg_index *idx, const float *d_queries, int64_t nq, int k, const uint8_t *mask)
{
    if (!idx->i4_nom.rows || (mask && !idx->i4_nom.int4_masked) || idx->dim % 32 != 0) return false;
    if (nq <= 128) {
        if (!idx->i4_nom.int4_small || nq < 5 || !int4_small_tile_fits(idx->dim)) return false;
        if (nq * idx->n < (mask ? kInt4NomMaskedSmallMinPairs : kInt4NomSmallMinPairs) && !hook(kHookInt4NomAlways)) return false;
    } else if (nq * idx->n < (mask ? kInt4NomMaskedMinPairs : kInt4NomMinPairs) && !hook(kHookInt4NomAlways)) {
        return false;
    }
    return k <= kNomMaxK && idx->n > k && aligned16(d_queries);
}
// nominated_pass with the INT4 re-score
int32_t int4_nominated_pass(vg_index *idx, const float *q, int64_t nq, int k, const uint8_t *mask, int64_t mask_stride, uint32_t *oid, float *osc,
                            hipStream_t st, std::vector<int> &failed)
{
    const NomImage &img = idx->i4_nom;
    const size_t before = failed.size();
    const Int4Row row{idx->d_int4_rows, idx->int4_table, idx->dim, reinterpret_cast<const float *>(img.rows), img.dim_pad};
    VG_TRY(nominated_pass(idx, img, false, q, nq, k, mask, mask_stride, 0, oid, osc, st, failed,
                          [&](const float *qq, int64_t cnt, const ProbeNominated &nom, float *, uint32_t *ids, float *scores, int *fail) -> int32_t {
                              return launch_nominated_verify<false>(row, qq, img.norm_max, cnt, nom, k, ids, scores, fail, st);
                          }));
    idx->i4_nom_rescanned += static_cast<int64_t>(failed.size() - before);  // (vg_index_int4_nomination_info)
    return VG_OK;
}
}  // namespace vg

VG_API int32_t vg_index_enable_int4_nomination(vg_index *idx, int32_t on, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_enable_int4_nomination: NULL index");
    // on & 3: the mode (1, or 2 with the small batches); on & 4: filtered batches too — of a mode, so 4 alone is none
    VG_CHECK(on != 4 && on <= 6, VG_ERR_INVALID_ARG, "vg_index_enable_int4_nomination: on=%d is a flag without a mode, or above 6", on);
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    VG_TRY(vg::nom_free(idx->i4_nom, st));
    if (!on) return VG_OK;
    VG_CHECK(idx->d_int4_rows && idx->int4_min && idx->int4_diff, VG_ERR_NOT_READY, "vg_index_enable_int4_nomination: index has no INT4 codes");
    idx->i4_nom_rescanned = 0;
    const int dim_pad = vg::nom_dim_pad(idx->dim);
    // mid, the scale and H2 in the rows' place (8 dim_pad + 4 bytes), the norms, norm_max
    VG_TRY(vg::nom_build(idx->i4_nom, idx->n, idx->dim, static_cast<int64_t>(2 * dim_pad + 1) * 4, true, st, [&](const vg::NomImage &b, int *norm_max_bits) {
        hipLaunchKernelGGL(vg::int4_mid_kernel, dim3(1), dim3(64), 0, st, idx->int4_min, idx->int4_diff, idx->dim, b.dim_pad, reinterpret_cast<float *>(b.rows));
        hipLaunchKernelGGL(vg::int4_codes_norms_kernel, dim3(static_cast<unsigned>((idx->n + 15) / 16)), dim3(256), 0, st, idx->d_int4_rows, idx->n, idx->dim,
                           idx->int4_min, idx->int4_diff, b.norms, norm_max_bits);
    }));
    idx->i4_nom.int4 = true;
    idx->i4_nom.int4_small = on > 0 && (on & 3) == 2;
    idx->i4_nom.int4_masked = on > 0 && (on & 4) != 0;
    idx->i4_nom.scale = reinterpret_cast<const float *>(idx->i4_nom.rows) + dim_pad;
    return VG_OK;
}

VG_API int32_t vg_index_int4_nomination_info(const vg_index *idx, int32_t *mode, int64_t *held_bytes, int64_t *rescanned)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_int4_nomination_info: NULL index");
    if (mode) *mode = !idx->i4_nom.rows ? 0 : (idx->i4_nom.int4_small ? 2 : 1) | (idx->i4_nom.int4_masked ? 4 : 0);
    if (held_bytes) *held_bytes = idx->i4_nom.held_bytes(idx->n);
    if (rescanned) *rescanned = idx->i4_nom.rows ? idx->i4_nom_rescanned : 0;
    return VG_OK;
}
