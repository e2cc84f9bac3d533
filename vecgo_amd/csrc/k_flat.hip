// k_flat.hip — exact brute-force search (flat/segment.go:691-721, hnsw.go:2021-2101):
//   1. scores[q][n] = ||x_n||^2 - 2 q.x_n  (L2)  or  -q.x_n  (Dot)   fp32 MFMA GEMM (above 128 queries: the split tile,
//      three bf16 products on the fp32 rows — gemm_runs_split; up to k = 16 behind a one-product screen whose proof, where it
//      holds, ends the query at step 3 — gemm_runs_screen)
//   2. per query: the kc smallest scores                              streaming select
//   3. exact re-scoring of those kc rows in the reference's summation order, top-k by
//      (Score, RowID), and a proof that no other row can belong to the top-k (k > 48: every row whose
//      GEMM score is under the query's threshold is re-scored, the proof is against the threshold)
//   4. queries whose proof fails are recomputed by the exhaustive exact kernel
// Steps 1-2 only nominate candidates; every reported id/score comes from step 3/4.
// The host side has each step once (GemmArgs, sample_thresholds, launch_flat_pick, launch_flat_verify) for its four drivers:
// flat_search_masked, flat_probe_gemm, flat_nominate_bf16, flat_thr_nominate; a driver's scratch is a struct that carves itself.
#include <algorithm>

#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "vg_cand_replay.hpp"
#include "vg_flat_gemm.hpp"
#include "vg_internal.hpp"
#include "vg_nominate.hpp"
#include "vg_search.hpp"

namespace vg {

// What the nomination GEMMs multiply: the fp32 queries and the n fp32 rows, or bfloat16 images of both (dim_words: 4-byte words per
// row).  `dma` picks the LDS-DMA kernels (16-byte aligned operands, dim % 4 == 0).  Filled by fp32_operands / gemm_operands.
struct GemmOperands {
    const float *a, *b;
    int64_t n;
    int dim_words;
    const float *norms;
    bool bf16, dma;
};
// One nomination's problem, shared by its GEMM launches: cnt queries against the rows, a row filter per query (mask + q *
// mask_stride: a bit per row), for the batch (stride 0) or none (k_probe.hip).
struct NomCall {
    hipStream_t st;
    bool dot;
    GemmOperands ops;
    int64_t cnt;
    const uint8_t *mask;
    int64_t mask_stride;
    unsigned ucnt() const { return static_cast<unsigned>(cnt); }
};
// One GEMM launch, built by name: sample() or append() of a problem, then the parts a launch has beyond them.
struct GemmArgs {
    const NomCall &c;
    const float *queries;  // c.ops.a, or the split tile's image of it
    float *scores = nullptr;
    int tile_stride = 1;
    int64_t out_cols = 0;
    const float *thr = nullptr;
    int thr_stride = 0, thr_off = 0;
    int *counts = nullptr;
    uint64_t *cand = nullptr;
    int cap = 0;
    int cus = 256;  // compute units of the device (the persistent bf16 tile launches one workgroup per CU)
    // nq * kCountLine ints of scratch: the persistent bf16 tile's counters, one 128-byte line per query.  An append is a returning
    // atomic on its query's counter; 1024 counters in 32 lines are 16 k atomics per line and launch, and a line serves them one
    // after the other (1024 queries x 1M x 768: 0.16 of the kernel's 1.35 ms went there — "keys stored without atomics" in
    // profiles/r06_gemm_bf16_probe.txt).  Null: the tile counts in `counts` itself.
    int *counts_wide = nullptr;
    // MODE 2, > 1: every skip_stride-th row tile is left out — the tiles MODE 1 sampled, whose passing rows the caller appends from
    // the sample itself (flat_sample_append_kernel).  Only where gemm_skips_sample() says so; 0: every tile.
    int skip_stride = 0;
    // MODE 2: the split tile (flat_gemm_split_big_kernel) — `queries` is flat_split_queries_kernel's image of the chunk, `base` the
    // fp32 rows.  Set only where gemm_runs_split() says so (vg_search_flat's fused path).  MODE 1: the sample on the same tile
    // (flat_gemm_sample_big_kernel), where sample_runs_big() says so — `queries` is that kernel's compact hi-only image.
    bool split = false;
    // with `split`: the screen (flat_gemm_screen_big_kernel), the product of the hi halves alone — where gemm_runs_screen() says so;
    // `queries` is the compact hi-only image
    bool screen = false;
    // with `split`, not `screen`: the retry behind a screen.  Bit tm of the word = query tile tm holds a query to retry; the others
    // are not multiplied.  flat_retry_prepare_kernel has written it and zeroed the counters of the queries to retry.
    const uint32_t *tile_active = nullptr;
    // MODE 2: the code-gathered tile (flat_gemm_codes_big_kernel) — c.ops.b is the decoded PQ codebook (NomImage::rows of a from_codes state), `codes` the
    // n rows' code bytes, code_m a row
    const uint8_t *codes = nullptr;
    int code_m = 0;
    // with `codes`: the SQ8 code tile (flat_gemm_sq8_big_kernel) — `codes` is the index's SQ8 code tiles, code_m their groups of 16
    // dimensions; c.ops.b is not read
    bool sq8 = false;

    explicit GemmArgs(const NomCall &call) : c(call), queries(call.ops.a) {}
    // MODE 0 / 1: the scores of every stride-th row tile into sc[cnt][cols] (stride 1: the whole score matrix)
    static GemmArgs sample(const NomCall &c, float *sc, int stride, int64_t cols)
    {
        GemmArgs a(c);
        a.scores = sc, a.tile_stride = stride, a.out_cols = cols;
        return a;
    }
    // MODE 2: every row scoring below its query's threshold thr[q * sel_k + sel_k - 1] appended to cand[q * cap ..], counted in counts[q]
    static GemmArgs append(const NomCall &c, const float *thr, int sel_k, int *counts, uint64_t *cand, int cap)
    {
        GemmArgs a(c);
        a.thr = thr, a.thr_stride = sel_k, a.thr_off = sel_k - 1, a.counts = counts, a.cand = cand, a.cap = cap;
        return a;
    }
    GemmArgs &wide(int *lines, int compute_units) { return counts_wide = lines, cus = compute_units, *this; }
    GemmArgs &skipping(int stride) { return skip_stride = stride, *this; }
    GemmArgs &split_tile(const uint32_t *image) { return queries = reinterpret_cast<const float *>(image), split = true, *this; }
    // (the screen and the sample read flat_split_queries_kernel's OTHER image, the compact hi-only one)
    GemmArgs &sample_tile(const uint32_t *hi_image) { return split_tile(hi_image); }
    GemmArgs &screen_tile(const uint32_t *hi_image) { return split_tile(hi_image), screen = true, *this; }
    GemmArgs &retry(const uint32_t *active) { return tile_active = active, *this; }
    GemmArgs &from_codes(const uint8_t *rows, int m) { return codes = rows, code_m = m, *this; }
    GemmArgs &from_sq8_codes(const uint8_t *tiles, int groups) { return codes = tiles, code_m = groups, sq8 = true, *this; }
};
constexpr int kCountLine = 32;
// Whether a MODE 2 launch of vg_search_flat's fused path runs the split tile: fp32 rows nominated by three bfloat16 products on the
// persistent 256 x 256 tile instead of the fp32 matrix instruction (16x the rate per product).  The ONE place that decides: the
// launcher, the query image and the proof's margin (split_gemm_eps) all follow it.  More than one 128-query tile, LDS-DMA operands
// (16-byte aligned), whole K steps of 32 floats, and the big tile's own limits (32-bit candidate offsets, 16-bit threshold stride).
// (test hook kHookFlatNoSplit: the fp32 GEMM as before)
static bool gemm_runs_split(bool fused, bool bf16, bool dma, int64_t nq, int dim, int cap, int thr_stride)
{
    return fused && !bf16 && dma && nq > kGemmBM && dim % kGemmBK == 0 && nq * static_cast<int64_t>(cap) < (int64_t(1) << 31) &&
           thr_stride < 65536 && !hook(kHookFlatNoSplit);
}
// The split tile's |score - true score| as a multiple of |q|^2 + max |x|^2 (the verify kernels' eps_extra).  With u = 2^-8
// (bfloat16 keeps 8 significant bits, round to nearest even) an operand is x = hi + lo + rho: hi = rne(x), the remainder
// r = x - hi exact in fp32 with |r| <= u |x|, lo = rne(r), so |lo| <= u |x| and |rho| <= u^2 |x|.  The tile sums
// q_hi x_hi + q_lo x_hi + q_hi x_lo, every product exact in fp32 (16 significant bits), and leaves out
//     q_lo x_lo + rho_q x + (q_hi + q_lo) rho_x:   at most (3 u^2 + u^4) |q_i x_i| per element,
// over a row (3 * 2^-16 + 2^-32) |q||x| <= 1.5001 * 2^-16 (|q|^2 + |x|^2).                                              [dropped]
// The accumulator starts at s = t (Dot) or (t - |x|^2) / 2 (L2), exact three-way splits summed by 8 matrix-unit additions, takes
// the 3 dim products, and the appended key's score is one more fma: m = 3 dim + 16 roundings, each taken to lose 2^-24 of the
// largest partial sum whatever the order: m 2^-24 (|s| + S), S = sum |products| <= (1 + u)^2 |q||x| <= 0.51 (|q|^2 + |x|^2).
// flat_thr_cap_kernel keeps t <= 2.002 (|q|^2 + max |x|^2) (a sampled threshold is a score and far inside), so |s| <= 2.002 of
// that for Dot and (2.002 + 1) / 2 <= 1.501 for L2.                                                                 [accumulation]
//     Dot:  1.5001 * 2^-16 + 2.52 (3 dim + 16) 2^-24          L2 (the score is -2 acc + ...: twice):  3.0002 * 2^-16 + 4.03 (3 dim + 16) 2^-24
// At dim 768: 1.7e-4 and 6.0e-4, beside the fp32 GEMM's own 4 dim 2^-24 = 1.8e-4 (kept: it also covers the exact re-score's
// roundings) and the bfloat16 filter's 8e-3.  tests/test_flat_split_bound.py models the sum and checks this function's formula.
// What the split cannot represent: |x| >= 2^128 (1 - 2^-9) rounds hi to Inf and lo to NaN, an Inf or NaN operand likewise —
// the accumulator of every product with it is NaN, and a NaN is never appended (the sign test is a float compare).  Such a row has
// |x|^2 = Inf or NaN, so d_norm_max is not finite and every query's margin eps is Inf or NaN: no proof holds and the exhaustive
// kernel answers, as under the bfloat16 filter; such a query has |q|^2 not finite, the same.  Denormals: a product or a lo half
// below 2^-126 that the matrix unit or the subtraction flushes moves the sum by at most 2^-126 dim max|q_i| < 1e-35 (1 + |q|^2),
// inside eps's absolute 1e-30 or its relative part.
static float split_gemm_eps(bool dot, int dim)
{
    const float m = static_cast<float>(3 * dim + 16) * 5.9604645e-8f;
    return dot ? 1.5001f * 1.52587890625e-5f + 2.52f * m : 3.0002f * 1.52587890625e-5f + 4.03f * m;
}
// The screen's (flat_gemm_screen_big_kernel, where gemm_runs_screen() says so) |score - true score| as a multiple of
// |q|^2 + max |x|^2.  With u = 2^-8 both operands are rounded to bfloat16, q_hi = q (1 + d), x_hi = x (1 + e), |d|, |e| <= u: a product is off by at most (2 u + u^2) |q_i x_i| = (2^-7 + 2^-16) |q_i x_i|,
// the dot product by (2^-7 + 2^-16) |q||x| <= (2^-8 + 2^-17) (|q|^2 + |x|^2); an L2 score is |x|^2 - 2 q.x, twice that — the
// bfloat16 filter's bound (vg_search_flat).                                                                          [operands]
// The accumulation is the split tile's with a third of the products: the same starting value s (|s| <= 2.002 for Dot, 1.501 for
// L2, by flat_thr_cap_kernel's cap), m = dim + 16 roundings (8 matrix-unit additions of the starting value, dim products, the
// key's fma; the rest is room), each at most 2^-24 (|s| + S), S = sum |products| <= (1 + u)^2 |q||x| <= 0.51 (|q|^2 + |x|^2):
//     Dot:  2^-8 + 2^-17 + 2.52 (dim + 16) 2^-24          L2:  2^-7 + 2^-16 + 4.03 (dim + 16) 2^-24                [accumulation]
// At dim 768 the L2 margin is 7.828e-3 + 1.88e-4 = 8.02e-3: the filter's "x 1.02" (7.97e-3, which has the 128 x 128 tile's
// zero-started sum to cover) is NOT enough for this tile from dim ~ 570 on, so the accumulation term is added as it is.
// tests/test_flat_screen_bound.py models the sum.  Values bfloat16 cannot hold: as for the split tile (split_gemm_eps).
static float screen_gemm_eps(bool dot, int dim)
{
    const float m = static_cast<float>(dim + 16) * 5.9604645e-8f;
    return dot ? 0.00390625f + 7.62939453125e-6f + 2.52f * m : 0.0078125f + 1.52587890625e-5f + 4.03f * m;
}
// The bfloat16 filter's (vg_index_enable_bf16_filter) share of a proof's margin, as a multiple of |q|^2 + max |x|^2: the
// nomination GEMMs read bf16 copies of the rows and of the queries; what they nominate is re-scored exactly as before and the
// proof widens its margin by the rounding the copies can introduce.  bfloat16 keeps 8 significant bits: rounding to nearest moves
// an operand by at most 2^-8 of its magnitude, a product q_i*x_i by at most (2^-7 + 2^-16)|q_i x_i|, the dot product by
// (2^-7 + 2^-16)|q||x| <= (2^-8 + 2^-17)(|q|^2 + |x|^2).  A Dot score is the dot product; an L2 score is
// |x|^2 - 2 q.x (norms from the fp32 rows), TWICE that: (2^-7 + 2^-16)(|q|^2 + |x|^2).  (r02 used the Dot
// bound for both — half of what L2 needs: ADVICE r02, tests/test_gpu_flat_bf16.py test_filter_worst_case_rounding.)
float bf16_filter_eps(bool dot) { return (dot ? 0.00390625f : 0.0078125f) * 1.02f; }
// Whether launch_gemm_t runs a kernel that honours GemmArgs::skip_stride for these arguments: the fp32 128 x 128 tiles (LDS-DMA and
// register-staged), whose MODE 1 and MODE 2 are one body with one accumulation order.  Not the 32-row tiles (up to 96 queries), not
// a bf16 kernel, not the split tile (`split`: gemm_runs_split's answer).  The ONE place that decides: the caller appends the sampled rows itself exactly where this is true (a row
// appended by both, or by neither, is a wrong answer).
static bool gemm_skips_sample(bool dma, int64_t nq, bool bf16, bool split = false)
{
    if (bf16 || split || hook(kHookFlatRescoreSample)) return false;
    return !(dma && nq <= 3 * kG32BM && !hook(kHookFlatNoSmallTile));
}
__global__ void counts_narrow_kernel(const int *__restrict__ wide, int64_t nq, int *__restrict__ counts)
{
    const int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q < nq) counts[q] = wide[q * kCountLine];
}

// a kernel that needs more dynamic LDS than the default 64 KiB: the attribute (on every call), the launch (none of an empty grid)
template <class Kern, class... Args>
static int32_t launch_lds(Kern kern, dim3 grid, dim3 threads, size_t lds, hipStream_t st, Args... args)
{
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    if (grid.x != 0) VG_LAUNCH(kern, grid, threads, lds, st, args...);
    return VG_OK;
}
// the 32-row tile of rb blocks of 32 query rows — fp32 rows: 1 .. 3, bf16 images: 1 .. 4 — as f(kernel, its LDS bytes)
template <bool DOT, int M, bool BF16, class F>
static int32_t with_g32_tile(int rb, F f)
{
    constexpr int kMost = BF16 ? 4 : 3;
    if (rb <= 1) return f(flat_gemm_dma32_kernel<DOT, M, 1, BF16>, g32_lds_bytes<1>());
    if (rb == 2) return f(flat_gemm_dma32_kernel<DOT, M, 2, BF16>, g32_lds_bytes<2>());
    if (rb == 3) return f(flat_gemm_dma32_kernel<DOT, M, 3, BF16>, g32_lds_bytes<3>());
    return f(flat_gemm_dma32_kernel<DOT, M, kMost, BF16>, g32_lds_bytes<kMost>());
}

template <bool DOT, int MODE>
static int32_t launch_gemm_t(const GemmArgs &a)
{
    const NomCall &c = a.c;
    const bool dma = c.ops.dma, bf16 = c.ops.bf16;
    const hipStream_t st = c.st;
    const int skip = MODE == 2 ? a.skip_stride : 0;
    VG_CHECK(skip == 0 || (skip > 1 && gemm_skips_sample(dma, c.cnt, bf16, a.split)), VG_ERR_INVALID_ARG, "launch_gemm: skip_stride on a kernel without it");
    // the grid of the 128 x 128 tiles: whole groups of 8 row tiles per query tile (the XCD-aware order); a sample launches every
    // tile_stride-th row tile, a launch with `skip` the tiles the sample left
    const int64_t mt = (c.cnt + kGemmBM - 1) / kGemmBM, nt = (c.ops.n + kGemmBN - 1) / kGemmBN;
    const int64_t tiles = skip ? nt - gemm_skip_sampled_tiles(nt, skip) : (nt + a.tile_stride - 1) / a.tile_stride;
    const dim3 grid(static_cast<unsigned>(mt * ((tiles + 7) / 8) * 8)), threads(kGemmThreads);
    // the persistent 256 x 256 tile (bf16 images, or the split tile on the fp32 rows): one workgroup per CU, wide counters
    // (extra: the split tile's tile_active.  A retry's counters are flat_retry_prepare_kernel's to zero: those of the queries it
    // retries, the others keep what the screen counted)
    auto big_grid = [&](int64_t bnt /* row tiles of 256 */) {
        const int64_t bmt = (c.cnt + kBigBM - 1) / kBigBM;
        const int64_t slots = bmt * ((bnt + 7) / 8) * 8, per_cu = std::max(a.cus / 8, 1) * 8;  // (one workgroup per CU: LDS)
        return dim3(static_cast<unsigned>(std::min(slots, per_cu)));
    };
    auto launch_big = [&](auto kern, size_t lds, auto... extra) -> int32_t {
        if (a.counts_wide && !a.tile_active) VG_HIP(hipMemsetAsync(a.counts_wide, 0, sizeof(int) * static_cast<size_t>(c.cnt) * kCountLine, st));
        VG_TRY(launch_lds(kern, big_grid((c.ops.n + kBigBN - 1) / kBigBN), dim3(kBigThreads), lds, st, a.queries, c.cnt, c.ops.b, c.ops.n,
                          c.ops.dim_words, c.ops.norms, a.thr, a.thr_stride, a.thr_off, a.counts_wide ? a.counts_wide : a.counts, a.cand, a.cap, c.mask,
                          c.mask_stride, a.counts_wide ? kCountLine : 1, extra...));
        if (a.counts_wide)
            VG_LAUNCH(counts_narrow_kernel, dim3(static_cast<unsigned>((c.cnt + 255) / 256)), dim3(256), 0, st, a.counts_wide, c.cnt, a.counts);
        return VG_OK;
    };
    // the 128 x 128 tiles (last: the row tiles a MODE 2 launch leaves out, 0 where the kernel has no such form) and the 32-row
    // tiles (one workgroup per row tile — of the sample: per sampled one)
    auto launch_tile = [&](auto kern, dim3 blocks, size_t lds, auto... last) -> int32_t {
        return launch_lds(kern, blocks, threads, lds, st, a.queries, c.cnt, c.ops.b, c.ops.n, c.ops.dim_words, c.ops.norms, a.scores, a.tile_stride, a.out_cols, a.thr,
                          a.thr_stride, a.thr_off, a.counts, a.cand, a.cap, c.mask, c.mask_stride, last...);
    };
    auto launch_128 = [&](auto kern, size_t lds, int last) { return launch_tile(kern, grid, lds, last); };
    auto launch_g32 = [&](auto kern, size_t lds) { return launch_tile(kern, dim3(static_cast<unsigned>(tiles)), lds); };
    constexpr int M = MODE == 0 ? 1 : MODE;
    const int rb = static_cast<int>((c.cnt + kG32BM - 1) / kG32BM);
    if constexpr (MODE == 1) {
        if (a.split) {  // the sample on the persistent tile: a row tile is a pair of sampled 128-row tiles
            VG_CHECK(!bf16 && gemm_runs_split(true, false, dma, c.cnt, c.ops.dim_words, 0, 0), VG_ERR_INVALID_ARG, "launch_gemm: sample tile on a call without it");
            return launch_lds(flat_gemm_sample_big_kernel<DOT, 3>, big_grid((tiles + 1) / 2), dim3(kBigThreads), big_lds_bytes<3, true>(), st, a.queries, c.cnt,
                              c.ops.b, c.ops.n, c.ops.dim_words, c.ops.norms, a.scores, a.tile_stride, a.out_cols, c.mask, c.mask_stride);
        }
    }
    if (MODE == 2 && a.split) {
        VG_CHECK(!bf16 && gemm_runs_split(true, false, dma, c.cnt, c.ops.dim_words, a.cap, a.thr_stride), VG_ERR_INVALID_ARG, "launch_gemm: split tile on a call without it");
        if (a.screen) return launch_big(flat_gemm_screen_big_kernel<DOT, 3>, big_lds_bytes<3, true>());
        VG_CHECK(!a.tile_active || (c.cnt <= 32 * kBigBM && a.counts_wide), VG_ERR_INVALID_ARG, "launch_gemm: tile_active is one word, with wide counters");
        note_flat_split_launch();
        return launch_big(flat_gemm_split_big_kernel<DOT, 3>, big_lds_bytes<3>(), a.tile_active);
    }
    if (MODE == 2 && a.codes && a.sq8) {  // (likewise; L2 and Dot)
        if constexpr (MODE == 2) {
            VG_CHECK(bf16 && c.cnt * static_cast<int64_t>(a.cap) < (int64_t(1) << 31) && a.thr_stride < 65536 && c.ops.dim_words % kGemmBK == 0 &&
                         a.code_m > 0 && c.ops.n > 0,
                     VG_ERR_INVALID_ARG, "launch_gemm: the SQ8 code tile on a call without it");
            return launch_big(flat_gemm_sq8_big_kernel<DOT, 3>, big_lds_bytes<3>(), a.codes, a.code_m);
        }
    }
    if (MODE == 2 && a.codes) {  // (any number of queries: there is no row image another tile could read)
        if constexpr (MODE == 2 && !DOT) {
            VG_CHECK(bf16 && c.cnt * static_cast<int64_t>(a.cap) < (int64_t(1) << 31) && a.thr_stride < 65536 && c.ops.dim_words % kGemmBK == 0,
                     VG_ERR_INVALID_ARG, "launch_gemm: the code-gathered tile on a call without it");
            return launch_big(flat_gemm_codes_big_kernel<false, 3>, big_lds_bytes<3>(), a.codes, a.code_m);
        }
        VG_CHECK(false, VG_ERR_INVALID_ARG, "launch_gemm: the code-gathered tile is L2's append");
    }
    if (skip && tiles == 0) return VG_OK;
    if (bf16) {  // rows of bfloat16 (c.ops.dim_words = 4-byte words per row): the LDS-DMA tiles only
        // up to 128 queries: the tile of 1 .. 4 blocks of 32 query rows (HBM-bound at the bf16 rate: 65 .. 128 queries 0.44 .. 0.49 ms on
        // the 128 x 128 tile, 0.40 .. 0.45 on this one — tools/mid_batch_time.py)
        if (c.cnt <= 4 * kG32BM && !hook(kHookFlatNoSmallTile)) return with_g32_tile<DOT, M, true>(rb, launch_g32);
        // more than one 128-query tile: the persistent 256 x 256 tile (32-bit candidate offsets: nq * cap < 2^31)
        if (MODE == 2 && c.cnt > kGemmBM && c.cnt * static_cast<int64_t>(a.cap) < (int64_t(1) << 31) && a.thr_stride < 65536 &&
            !hook(kHookFlatNoBigTile)) {
            const bool two = hook(kHookFlatBigTile2);
            auto kern = two ? flat_gemm_bf16_big_kernel<DOT, 2> : hook(kHookFlatBigEarlyB) ? flat_gemm_bf16_big_kernel<DOT, 3, 512> : flat_gemm_bf16_big_kernel<DOT, 3>;
            return launch_big(kern, two ? big_lds_bytes<2>() : big_lds_bytes<3>());
        }
        return launch_128(flat_gemm_dma_kernel<DOT, M, 0, true>, kDmaLdsBytes, 0);
    }
    // (test hook kHookFlatNoSmallTile: always the 128-query tile)
    // 1 - 3 blocks of 32 queries: the HBM-bound shapes, and 65 .. 96 queries at three quarters of the 128-query tile's matrix work
    // (1.65 -> 1.28 ms per call at 1M x 768; 97 .. 128 queries: four blocks run as long as the 128 x 128 tile, which keeps them)
    if (dma && MODE != 0 && c.cnt <= 3 * kG32BM && !hook(kHookFlatNoSmallTile)) return with_g32_tile<DOT, M, false>(rb, launch_g32);
    if (dma) return launch_128(flat_gemm_dma_kernel<DOT, MODE>, kDmaLdsBytes, skip);
    return launch_128(flat_gemm_kernel<DOT, MODE>, kGemmLdsBytes, skip);
}

template <int MODE>
static int32_t launch_gemm(const GemmArgs &a)
{
    return a.c.dot ? launch_gemm_t<true, MODE>(a) : launch_gemm_t<false, MODE>(a);
}

// fp32 -> bfloat16, round to nearest even (NaN stays NaN): rows of `dim` floats written as rows of `dim_pad` bfloat16, the tail
// zeros (operands of the bf16 GEMM are padded to whole K steps)
__device__ __forceinline__ uint16_t bf16_rne_bits(uint32_t u)
{
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu) != 0) return static_cast<uint16_t>((u >> 16) | 0x0040u);
    return static_cast<uint16_t>((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__global__ void f32_to_bf16_pad_kernel(const float *__restrict__ src, int64_t rows, int dim, int dim_pad, uint16_t *__restrict__ dst)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= rows * dim_pad) return;
    const int64_t r = i / dim_pad;
    const int j = static_cast<int>(i - r * dim_pad);
    dst[i] = bf16_rne_bits(j < dim ? __float_as_uint(src[r * dim + j]) : 0u);
}
// the same of src[r][j] * scale[j] — one fp32 rounding, then the bfloat16 one: the queries of the SQ8 nomination from the codes
__global__ void f32_scaled_to_bf16_pad_kernel(const float *__restrict__ src, const float *__restrict__ scale, int64_t rows, int dim, int dim_pad,
                                              uint16_t *__restrict__ dst)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= rows * dim_pad) return;
    const int64_t r = i / dim_pad;
    const int j = static_cast<int>(i - r * dim_pad);
    dst[i] = bf16_rne_bits(j < dim ? __float_as_uint(src[r * dim + j] * scale[j]) : 0u);
}

// The queries of the split tile (flat_gemm_split_big_kernel) as an image of `dim` 4-byte words per row, like the fp32 row it is
// made from: every 128-byte K step holds [hi of its 32 elements | lo of the same 32], so that both operands advance by the same
// k per step.  One thread per pair of elements; dim % 32 == 0.
// Beside it `hi_dst`, the compact image the screen and the sample on its tile read (flat_gemm_big_body, OPS = kBigScreen): the same
// hi words and nothing else, blocked per (256-query tile, K step) in the tile's LDS order — block (tile, step) is 256 rows of
// 16 words, slot (4 words) s of row R = granule s ^ ((R >> 2) & 3) of the step — so that a fill piece is one contiguous KiB.
// It holds WHOLE tiles (flat_hi_image_rows): a row past `rows` is the last query's, which is what the tile's fills used to
// re-read for it.  The grid covers the padded rows.
static int64_t flat_hi_image_rows(int64_t rows) { return (rows + kBigBM - 1) / kBigBM * kBigBM; }
__global__ void flat_split_queries_kernel(const float *__restrict__ src, int64_t rows, int dim, uint32_t *__restrict__ dst,
                                          uint32_t *__restrict__ hi_dst)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;  // pair index
    const int half = dim / 2;
    const int64_t r = i / half;
    if (r >= (rows + kBigBM - 1) / kBigBM * kBigBM) return;
    const int64_t rs = r < rows ? r : rows - 1;
    const int p = static_cast<int>(i - r * half), s = p >> 4, w = p & 15;
    const float2 v = *reinterpret_cast<const float2 *>(src + rs * dim + 32 * s + 2 * w);
    uint32_t hi, lo;
    split2_bf16(v.x, v.y, hi, lo);
    if (r < rows) {
        dst[r * dim + 32 * s + w] = hi;
        dst[r * dim + 32 * s + 16 + w] = lo;
    }
    const int R = static_cast<int>(r & (kBigBM - 1));
    hi_dst[((r / kBigBM) * (dim / 32) + s) * (kBigBM * 16) + R * 16 + (((w >> 2) ^ ((R >> 2) & 3)) << 2) + (w & 3)] = hi;
}

// After the proofs: the work list of step 4 (todo[0] = how many queries need the exhaustive scan,
// todo[1 + j] = the j-th of them, ascending) and the bookkeeping for vg_index_flat_stats
// (stats[0] += queries of the chunk, stats[1] += those sent to the exhaustive kernel; counts, or null: stats[3] += the sum of
// the chunk's candidate counts, what the fused path appended — vg_index_flat_appended).
__global__ __launch_bounds__(256) void flat_todo_kernel(const int *__restrict__ flags, const int *__restrict__ always,
                                                        int cnt, int *__restrict__ todo,
                                                        unsigned long long *__restrict__ stats, const int *__restrict__ counts)
{
    __shared__ int part[256];
    __shared__ unsigned long long appended[256];
    const int tid = threadIdx.x;
    const int per = (cnt + 255) / 256;
    const int lo = tid * per < cnt ? tid * per : cnt, hi = lo + per < cnt ? lo + per : cnt;
    if (!flags) {  // a path with no proof step: only count the queries
        if (tid == 0) atomicAdd(&stats[0], static_cast<unsigned long long>(cnt));
        return;
    }
    const bool all = *always != 0;
    int mine = 0;
    unsigned long long app = 0;
    for (int i = lo; i < hi; i++) {
        mine += (all || flags[i] != 0);
        if (counts) app += static_cast<unsigned long long>(counts[i]);
    }
    part[tid] = mine;
    appended[tid] = app;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        app = 0;
        for (int t = 0; t < 256; t++) {
            const int c = part[t];
            part[t] = run;
            run += c;
            app += appended[t];
        }
        todo[0] = run;
        if (counts) atomicAdd(&stats[3], app);
        atomicAdd(&stats[0], static_cast<unsigned long long>(cnt));
        atomicAdd(&stats[1], static_cast<unsigned long long>(run));
    }
    __syncthreads();
    int at = part[tid];
    for (int i = lo; i < hi; i++)
        if (all || flags[i] != 0) todo[1 + at++] = i;
}

// Between the screen's proofs and the split tile's retry (vg_search_flat): a query whose flag is set is retried — its counters
// (narrow and wide) go back to zero, its threshold stays, its 256-query tile is marked in the word *tile_active — and every other
// query of the chunk gets the threshold -Inf, for which the tile's clamp appends nothing.  all: every query counts as flagged
// (test hook kHookFlatScreenFail).  stats[2] += the queries retried.  ONE workgroup, a round per query tile (at most 32: the
// word is written whole, no memset and no atomics in front of it).
__global__ __launch_bounds__(kBigBM) void flat_retry_prepare_kernel(int *__restrict__ flags, bool all, int cnt, float *__restrict__ thr,
                                                                    int thr_stride, int thr_off, int *__restrict__ counts,
                                                                    int *__restrict__ counts_wide, uint32_t *__restrict__ tile_active,
                                                                    unsigned long long *__restrict__ stats)
{
    uint32_t word = 0;
    int total = 0;
    for (int t = 0; t * kBigBM < cnt; t++) {
        const int q = t * kBigBM + static_cast<int>(threadIdx.x);
        bool retry = false;
        if (q < cnt) {
            retry = all || flags[q] != 0;
            if (retry) {
                flags[q] = 1;
                counts[q] = 0;
                counts_wide[static_cast<int64_t>(q) * kCountLine] = 0;
            } else {
                thr[static_cast<int64_t>(q) * thr_stride + thr_off] = -INFINITY;
            }
        }
        const int here = __syncthreads_count(retry);
        word |= here ? 1u << t : 0u;
        total += here;
    }
    if (threadIdx.x == 0) {
        *tile_active = word;
        if (total) atomicAdd(&stats[2], static_cast<unsigned long long>(total));
    }
}

// The sampled row tiles are scored once.  MODE 1 has left their scores in sc[q][ns] (+Inf for a column past n and for a row the
// query's filter rejects); MODE 2 of the same 128 x 128 tile would compute the same bits again and compare them with the query's
// threshold.  So, once the thresholds exist: one workgroup per query walks its sample, appends key(sc, row) for every column with
// sc < threshold — column c = row (c / 128) * sample_stride * 128 + c % 128 — and SETS counts[q] to how many passed (those past
// `cap` too: the overflow test wants the full count), which also stands in for the memset in front of the main GEMM; that GEMM
// then leaves the sampled tiles out (GemmArgs::skip_stride).  Slots: a ballot prefix per wave, the waves' totals through LDS (no
// atomics; the order of a list's keys means nothing).  A round is 4096 columns — four 16-byte loads per thread, all issued before
// the first compare (one load per thread and round: 62 rounds of a load's latency and a barrier at 1M rows).
constexpr int kSampleAppendThreads = 256, kSampleAppendVec = 4;
__global__ __launch_bounds__(kSampleAppendThreads) void flat_sample_append_kernel(
    const float *__restrict__ sc /* 16-byte aligned, ns % 4 == 0 */, int64_t ns, int sample_stride, const float *__restrict__ thr,
    int thr_stride, int thr_off, int *__restrict__ counts, uint64_t *__restrict__ cand, int cap)
{
    constexpr int kWaves = kSampleAppendThreads / 64, kPiece = kSampleAppendThreads * 4, kRound = kPiece * kSampleAppendVec;
    __shared__ int wave_n[2][kWaves];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float t = thr[q * thr_stride + thr_off];
    const float *row = sc + q * ns;
    uint64_t *dst = cand + q * cap;
    const uint64_t below = (uint64_t(1) << lane) - 1;
    int run = 0;  // passed so far (uniform over the workgroup)
    for (int64_t c0 = 0, round = 0; c0 < ns; c0 += kRound, round++) {
        float v[kSampleAppendVec][4];
#pragma unroll
        for (int u = 0; u < kSampleAppendVec; u++) {
            const int64_t c = c0 + u * kPiece + tid * 4;
            const float4 x = c < ns ? *reinterpret_cast<const float4 *>(row + c) : make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
            v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
        }
        int mine = 0;  // this wave's
#pragma unroll
        for (int u = 0; u < kSampleAppendVec; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) mine += __popcll(__ballot(v[u][e] < t));
        const int b = static_cast<int>(round & 1);  // two sets of totals: one barrier per round
        if (lane == 0) wave_n[b][wave] = mine;
        __syncthreads();
        int at = run, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            const int cnt = wave_n[b][w];
            at += w < wave ? cnt : 0;
            all += cnt;
        }
        if (mine != 0) {  // (uniform over the wave)
#pragma unroll
            for (int u = 0; u < kSampleAppendVec; u++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const bool pass = v[u][e] < t;
                    const uint64_t bal = __ballot(pass);
                    const int pos = at + __popcll(bal & below);
                    const int64_t c = c0 + u * kPiece + tid * 4 + e;
                    if (pass && pos < cap)
                        dst[pos] = make_key(v[u][e], static_cast<uint32_t>((c / kGemmBN) * sample_stride * kGemmBN + c % kGemmBN), false);
                    at += __popcll(bal);
                }
        }
        run += all;
    }
    if (tid == 0) counts[q] = run;
}

// per query: the kc best keys among the candidates the fused GEMM appended (count <= cap)
// only (or null: every query): the workgroup of a query with only[q] == 0 returns at once and writes nothing
__global__ __launch_bounds__(256) void flat_pick_kernel(const uint64_t *__restrict__ cand,
                                                        const int *__restrict__ counts, int cap, int kc,
                                                        uint32_t *__restrict__ cand_ids,
                                                        float *__restrict__ cand_scores, const int *__restrict__ only)
{
    __shared__ uint64_t lists[4 * 64];
    __shared__ int valid[4];
    __shared__ uint64_t best[64];
    const int64_t q = blockIdx.x;
    if (only && only[q] == 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int c = counts[q];
    if (c > cap) c = cap;
    const uint64_t *src = cand + q * cap;
    WaveTopK tk;
    tk.init(kc);
    for (int i0 = wave * 64; i0 < c; i0 += 256) {
        const int i = i0 + lane;
        tk.offer(i < c ? src[i] : kKeyMax, lane);
    }
    wg_rank_merge<4>(tk, lists, valid, wave, lane, tid, kc, best);
    __syncthreads();
    if (tid < kc) {
        const uint64_t e = best[tid];
        cand_ids[q * kc + tid] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        cand_scores[q * kc + tid] = e == kKeyMax ? INFINITY : key_score(e, false);
    }
}

__global__ void fill_f32_kernel(float *p, int64_t n, float v)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// A query's thresholds never above the largest score a row can have: 2 (|q|^2 + max |x|^2) >= |x|^2 + 2 |q| |x| (L2) >= |q.x|
// (Dot), with room for the bfloat16 rounding of both operands.  "No threshold" (+Inf: no sample of a small segment, a filter that
// leaves the sample short) means the same after it — every row passes — but the persistent bf16 tile (flat_gemm_bf16_big_kernel)
// starts its accumulators at (t - |x|^2) / 2 and reads a row's score back as t - 2 acc: with t = 1e30 standing in for +Inf the dot
// product is absorbed, every appended score comes back as ~0, and the 64 "best" of them were an arbitrary 64 (r06: Dot segments of
// up to 4096 rows, batches above 128 queries, answered wrongly — tests/test_gpu_nonfinite.py found it).  One wave per query.
__global__ __launch_bounds__(64) void flat_thr_cap_kernel(float *__restrict__ thr, int sel_k, const float *__restrict__ queries, int dim,
                                                          const float *__restrict__ norm_max)
{
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    float qn = 0.0f;
    for (int j = lane; j < dim; j += 64) qn = __builtin_fmaf(queries[q * dim + j], queries[q * dim + j], qn);
    for (int off = 32; off > 0; off >>= 1) qn += __shfl_xor(qn, off);
    const float bound = 2.002f * (qn + norm_max[0]);
    if (!(bound < 1e30f)) return;  // not finite: the tile's own clamp stands in, and every proof fails on its (infinite) margin
    for (int i = lane; i < sel_k; i += 64) {
        const float t = thr[q * sel_k + i];
        if (!(t < bound)) thr[q * sel_k + i] = bound;  // (NaN too)
    }
}

// ---- 2. per-query streaming select of the kc smallest scores -------------------------------
constexpr int kSelWaves = 4;
constexpr int kSelThreads = kSelWaves * 64;
__global__ __launch_bounds__(kSelThreads) void flat_select_kernel(const float *__restrict__ scores,
                                                                  int64_t n, int slices, int kc,
                                                                  uint64_t *__restrict__ partial)
{
    __shared__ uint64_t lists[kSelWaves * 64];
    __shared__ int valid[kSelWaves];
    const int s = blockIdx.x;
    const int64_t q = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = n * s / slices, r1 = n * (s + 1) / slices;
    const float *row = scores + q * n;
    WaveTopK tk;
    tk.init(kc);
    // each wave sweeps chunks of 64 lanes x 4 loads x 4 floats; the 4 loads are unguarded and in
    // flight together (a guarded load would serialise on vmcnt(0)); a chunk whose minimum is not
    // below the wave's k-th key is skipped with one ballot
    const int64_t a0 = (r0 + 3) & ~int64_t(3);          // 16-byte aligned interior [a0, a1)
    const int64_t a1 = a0 + ((r1 - a0) / 1024) * 1024;  // whole 1024-float chunks
    if (a0 < r1 && a1 > a0) {
        const float4 *row4 = reinterpret_cast<const float4 *>(row + a0);
        const int64_t chunks = (a1 - a0) / 1024;
        for (int64_t c = wave; c < chunks; c += kSelWaves) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = row4[c * 256 + u * 64 + lane];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t i = a0 + c * 1024 + (u * 64 + lane) * 4;
                const float vals[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                float mn = fminf(fminf(vals[0], vals[1]), fminf(vals[2], vals[3]));
                if (!__ballot(make_key(mn, 0u, false) < tk.tau)) continue;
#pragma unroll
                for (int e = 0; e < 4; e++)
                    tk.offer(make_key(vals[e], static_cast<uint32_t>(i + e), false), lane);
            }
        }
    }
    // ragged head and tail
    {
        const int64_t head_end = (a0 < r1 && a1 > a0) ? a0 : r1;
        for (int64_t i0 = r0 + wave * 64; i0 < head_end; i0 += kSelThreads) {
            const int64_t i = i0 + lane;
            tk.offer(i < head_end ? make_key(row[i], static_cast<uint32_t>(i), false) : kKeyMax, lane);
        }
        const int64_t tail_begin = (a0 < r1 && a1 > a0) ? a1 : r1;
        for (int64_t i0 = tail_begin + wave * 64; i0 < r1; i0 += kSelThreads) {
            const int64_t i = i0 + lane;
            tk.offer(i < r1 ? make_key(row[i], static_cast<uint32_t>(i), false) : kKeyMax, lane);
        }
    }
    wg_rank_merge<kSelWaves>(tk, lists, valid, wave, lane, tid, kc,
                             partial + (q * slices + s) * kc);
}

// ---- 3. exact re-score + proof -----------------------------------------------------------------
// cand_ids/cand_scores: the kc best GEMM scores per query, ascending.  One workgroup per query.
// only (or null: every query; may be `fallback` itself): the workgroup of a query with only[q] == 0 returns at once and writes
// nothing — the second proof of the queries whose first one failed rewrites their flag and leaves the others' answers alone.
template <bool DOT>
__global__ __launch_bounds__(256) void flat_verify_kernel(
    const float *__restrict__ base, int64_t n, int dim, const float *__restrict__ queries,
    const float *__restrict__ norms_max /* [1] */, const uint32_t *__restrict__ cand_ids,
    const float *__restrict__ cand_scores, int kc, int k, uint32_t *__restrict__ ids,
    float *__restrict__ scores, int *fallback, const float *__restrict__ thr, int thr_stride,
    int thr_off, const int *__restrict__ counts, int cap, float eps_extra, const int *only)
{
    __shared__ uint64_t keys[64];
    const Sub16 sub = Sub16::make(threadIdx.x);
    const int64_t q = blockIdx.x;
    if (only && only[q] == 0) return;
    const float *qv = queries + q * dim;
    for (int c = threadIdx.x >> 4; c < kc; c += 16) {
        const uint32_t id = cand_ids[q * kc + c];
        uint64_t key = kKeyMax;
        if (id != VG_INVALID_ID) {
            const float v = exact_pair16<DOT, kPair>(base + static_cast<int64_t>(id) * dim, qv, dim, sub);
            key = make_key(v, id, DOT);
        }
        if ((threadIdx.x & 15) == 0) keys[c] = key;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    WaveTopK tk;
    tk.init(k);
    tk.offer(lane < kc ? keys[lane] : kKeyMax, lane);
    // ||q||^2 (any order: only feeds the error bound)
    float qn = 0.0f;
    for (int j = lane; j < dim; j += 64) qn = __builtin_fmaf(qv[j], qv[j], qn);
    for (int off = 32; off > 0; off >>= 1) qn += __shfl_xor(qn, off);
    const uint64_t kth = readlane_u64(tk.list, k - 1);
    bool ok = true;
    // tau: a lower bound on the GEMM score of every row that was NOT nominated
    float tau;
    bool have_all;
    if (thr) {  // fused path: rows not appended have score >= threshold; appended-but-not-picked
                // rows have score >= the kc-th picked score
        const float tq = thr[q * thr_stride + thr_off];
        const int cnt = counts[q];
        if (cnt > cap) ok = false;  // buffer overflow: some rows below the threshold were dropped
        tau = cnt > kc ? fminf(tq, cand_scores[q * kc + (kc - 1)]) : tq;
        have_all = (tq == INFINITY) && cnt <= kc;
    } else {
        tau = cand_scores[q * kc + (kc - 1)];  // worst nominated GEMM score
        have_all = (n <= kc);                  // every row is a candidate: nothing to prove
    }
    if (ok && !have_all) {
        const float xmax = norms_max[0];
        // fp32 GEMM-form vs exact: |err| <= ~ 2*dim*2^-24*(|q||x|) per dot; bound generously
        // (eps_extra: the bf16 filter's share, 0 for the fp32 GEMM — see vg_index_enable_bf16_filter)
        const float eps = (4.0f * (static_cast<float>(dim) * 5.9604645e-8f) + eps_extra) * (qn + xmax) + 1e-30f;
        if (tau == INFINITY) {
            ok = true;  // nothing was excluded
        } else if (kth == kKeyMax) {
            ok = false;
        } else if (DOT) {
            // outside rows: -q.x >= tau  =>  q.x <= -tau (+eps); need kth dot > that
            const float dk = key_score(kth, true);
            ok = dk > (-tau) + eps;
        } else {
            const float dk = key_score(kth, false);
            ok = dk < (tau + qn) - eps;
        }
    }
    if (lane < k) {
        const uint64_t e = tk.list;
        ids[q * k + lane] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        scores[q * k + lane] = e == kKeyMax ? (DOT ? -INFINITY : INFINITY) : key_score(e, DOT);
    }
    if (lane == 0) fallback[q] = ok ? 0 : 1;
}

// The same for k beyond the 64-candidate budget: EVERY appended row (GEMM score below the query's
// threshold, ~500 of them) is re-scored exactly, so the only rows left to argue about are the ones the
// threshold excluded: the proof compares the k-th exact score with the threshold itself.
template <bool DOT>
__global__ __launch_bounds__(256) void flat_verify_all_kernel(
    const float *__restrict__ base, int dim, const float *__restrict__ queries,
    const float *__restrict__ norms_max /* [1] */, const uint64_t *__restrict__ cand, const int *__restrict__ counts,
    int cap, int k, uint32_t *__restrict__ ids, float *__restrict__ scores, int *__restrict__ fallback,
    const float *__restrict__ thr, int thr_stride, int thr_off, float eps_extra)
{
    __shared__ uint64_t lists[4 * 64];
    __shared__ int valid[4];
    __shared__ uint64_t best[64];
    const Sub16 sub = Sub16::make(threadIdx.x);
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *qv = queries + q * dim;
    const int total = counts[q];
    const int cnt = total < cap ? total : cap;
    WaveTopK tk;
    tk.init(k);
    for (int c0 = wave * 4; c0 < cnt; c0 += 16) {  // 4 candidates per wave step, one per 16-lane group
        const int c = c0 + (lane >> 4);
        uint64_t key = kKeyMax;
        if (c < cnt) {
            const uint32_t id = key_row(cand[q * cap + c]);
            const float v = exact_pair16<DOT, kPair>(base + static_cast<int64_t>(id) * dim, qv, dim, sub);
            if ((lane & 15) == 0) key = make_key(v, id, DOT);
        }
        tk.offer(key, lane);
    }
    wg_rank_merge<4>(tk, lists, valid, wave, lane, tid, k, best);
    __syncthreads();
    if (tid >= 64) return;
    float qn = 0.0f;  // ||q||^2 (any order: only feeds the error bound)
    for (int j = lane; j < dim; j += 64) qn = __builtin_fmaf(qv[j], qv[j], qn);
    for (int off = 32; off > 0; off >>= 1) qn += __shfl_xor(qn, off);
    const uint64_t kth = best[k - 1];
    const float tau = thr[q * thr_stride + thr_off];  // every row that was not appended scores >= tau
    bool ok = total <= cap;                           // overflow: rows below the threshold were dropped
    if (ok && tau != INFINITY) {
        const float xmax = norms_max[0];
        // (eps_extra: the bf16 filter's share, 0 for the fp32 GEMM — see vg_index_enable_bf16_filter)
        const float eps = (4.0f * (static_cast<float>(dim) * 5.9604645e-8f) + eps_extra) * (qn + xmax) + 1e-30f;
        if (kth == kKeyMax)
            ok = false;
        else if (DOT)
            ok = key_score(kth, true) > (-tau) + eps;
        else
            ok = key_score(kth, false) < (tau + qn) - eps;
    }
    if (lane < k) {
        const uint64_t e = best[lane];
        ids[q * k + lane] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        scores[q * k + lane] = e == kKeyMax ? (DOT ? -INFINITY : INFINITY) : key_score(e, DOT);
    }
    if (lane == 0) fallback[q] = ok ? 0 : 1;
}

// k > 64 (one wave's register list holds 64 keys): the exact keys of every appended row are sorted in
// LDS instead; the proof is the same as above.  n2 = the power of two the workgroup sorts (>= appended rows).
template <bool DOT>
__global__ __launch_bounds__(256) void flat_verify_sort_kernel(
    const float *__restrict__ base, int dim, const float *__restrict__ queries,
    const float *__restrict__ norms_max /* [1] */, const uint64_t *__restrict__ cand, const int *__restrict__ counts,
    int cap, int k, uint32_t *__restrict__ ids, float *__restrict__ scores, int *__restrict__ fallback,
    const float *__restrict__ thr, int thr_stride, int thr_off, float eps_extra)
{
    extern __shared__ uint64_t sortbuf[];  // cap keys
    const Sub16 sub = Sub16::make(threadIdx.x);
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const float *qv = queries + q * dim;
    const int total = counts[q];
    const int cnt = total < cap ? total : cap;
    int n2 = 64;
    while (n2 < cnt) n2 <<= 1;
    for (int c0 = 0; c0 < cnt; c0 += 16) {  // 16 candidates per step, one per 16-lane group
        const int c = c0 + (tid >> 4);
        if (c < cnt) {
            const uint32_t id = key_row(cand[q * cap + c]);
            const float v = exact_pair16<DOT, kPair>(base + static_cast<int64_t>(id) * dim, qv, dim, sub);
            if ((tid & 15) == 0) sortbuf[c] = make_key(v, id, DOT);
        }
    }
    for (int i = cnt + tid; i < n2; i += 256) sortbuf[i] = kKeyMax;
    __syncthreads();
    bitonic_sort_lds(sortbuf, n2, tid, 256);
    for (int i = tid; i < k; i += 256) {
        const uint64_t e = i < n2 ? sortbuf[i] : kKeyMax;
        ids[q * k + i] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        scores[q * k + i] = e == kKeyMax ? (DOT ? -INFINITY : INFINITY) : key_score(e, DOT);
    }
    if (tid >= 64) return;
    float qn = 0.0f;
    for (int j = lane; j < dim; j += 64) qn = __builtin_fmaf(qv[j], qv[j], qn);
    for (int off = 32; off > 0; off >>= 1) qn += __shfl_xor(qn, off);
    const uint64_t kth = k - 1 < n2 ? sortbuf[k - 1] : kKeyMax;
    const float tau = thr[q * thr_stride + thr_off];
    bool ok = total <= cap;
    if (ok && tau != INFINITY) {
        const float xmax = norms_max[0];
        // (eps_extra: the bf16 filter's share, 0 for the fp32 GEMM — see vg_index_enable_bf16_filter)
        const float eps = (4.0f * (static_cast<float>(dim) * 5.9604645e-8f) + eps_extra) * (qn + xmax) + 1e-30f;
        if (kth == kKeyMax)
            ok = false;
        else if (DOT)
            ok = key_score(kth, true) > (-tau) + eps;
        else
            ok = key_score(kth, false) < (tau + qn) - eps;
    }
    if (lane == 0) fallback[q] = ok ? 0 : 1;
}

// ---- 4. exhaustive exact scan for the queries whose proof failed ---------------------------------
// grid = (slices, slots): slot y takes the work-list entries y, y + slots, ...; with an empty list
// (the normal case) the whole launch is a few thousand workgroups that read one word and leave.
constexpr int kExactSlots = 32;
template <bool DOT>
__global__ __launch_bounds__(256) void flat_exact_kernel(const float *__restrict__ base, int64_t n,
                                                         int dim, const float *__restrict__ queries,
                                                         const int *__restrict__ todo, int slices, int k,
                                                         uint64_t *__restrict__ partial,
                                                         const uint64_t *__restrict__ min_keys = nullptr,
                                                         const uint8_t *__restrict__ mask = nullptr, int64_t mask_stride = 0)
{
    __shared__ uint64_t lists[4 * 64];
    __shared__ int valid[4];
    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntodo = todo[0];
    const Sub16 sub = Sub16::make(tid);
    const int64_t r0 = n * s / slices, r1 = n * (s + 1) / slices;
    for (int j = blockIdx.y; j < ntodo; j += gridDim.y) {
        const int64_t q = todo[1 + j];
        uint64_t *out = partial + (q * slices + s) * k;
        const float *qv = queries + q * dim;
        // paged results (k > 64): only keys after the last one of the previous page count
        const uint64_t floor_key = min_keys ? min_keys[q] : 0;
        const uint8_t *mq = mask ? mask + q * mask_stride : nullptr;  // filtered search: rows the filter rejects are skipped
        WaveTopK tk;
        tk.init(k);
        // 4 rows per wave step (one per 16-lane group)
        for (int64_t i0 = r0 + wave * 4; i0 < r1; i0 += 16) {
            const int64_t i = i0 + (lane >> 4);
            uint64_t key = kKeyMax;
            if (i < r1 && mask_bit(mq, i)) {
                const float v = exact_pair16<DOT, kPair>(base + i * dim, qv, dim, sub);
                if ((lane & 15) == 0) {
                    key = make_key(v, static_cast<uint32_t>(i), DOT);
                    if (min_keys && key <= floor_key) key = kKeyMax;
                }
            }
            tk.offer(key, lane);
        }
        wg_rank_merge<4>(tk, lists, valid, wave, lane, tid, k, out);
        __syncthreads();  // lists / valid are reused by the next work item
    }
}

// ---- small query batches: one HBM pass scores every row against up to 8 queries --------------------
// Below ~5 queries even the 32-query GEMM tile is slower than a plain scan (a 128-query tile does 128 queries'
// worth of MFMA work and 1/8 of the tiles' loads for whatever is in it: 1.65 ms at 1M x 768).
// This kernel is the HBM-bound alternative: a 16-lane group loads a row ONCE into registers
// (dim <= 1024: 16 float4 per lane) and scores it against QB queries held in LDS, each in the
// reference's summation order (vg_exact.hpp, kPair) — exact by construction, no proof step.
constexpr int kScanQB = 8;        // queries one pass can carry
constexpr int kGemmMaxK = 48;     // largest k the 64-candidate nomination + proof serves (above: flat_verify_all_kernel)
constexpr int kFlatMaxK = 512;    // candidates appended per query stay well under the 4096-key buffer (3k expected)
// Whether a chunk that runs the split tile (gemm_runs_split's answer) is screened first: one product, q_hi.x_hi, over every pair,
// its proof with the wide margin screen_gemm_eps, and the three-product tile only for the 256-query tiles that hold a query whose
// proof failed.  The ONE place that decides.  The cascade serves the proof from 64 picked candidates (k <= kGemmMaxK: the other
// verify kernels keep the split tile alone), but the screen's proof wants the k-th neighbour further below the 64th than its
// margin, ~2^-7 (|q|^2 + max |x|^2), and on unclustered rows that holds only while k is a small part of the 64: standard-normal
// rows (5000 x 32 .. 768, tests/test_gpu_flat_screen.py's data, on the GPU and in a numpy model of the proof) leave no query
// open up to k = 24, 12 % of them at k = 32 (dim 768) and 13 % (dim 32) to all of them (dim 768) at k = 48 — where the screen
// is a pass for nothing in front of the three-product pass.  So: up to kScreenMaxK = 16 results, a quarter of the candidates.
// (test hooks: kHookFlatNoScreen — no screen, the split tile for every tile; kHookFlatNoSplit turns both off;
// kHookFlatScreenFail, which fails every screen proof, also runs the screen up to kGemmMaxK so that the retry is tested there)
constexpr int kScreenMaxK = 16;
static bool gemm_runs_screen(bool split, int k)
{
    return split && !hook(kHookFlatNoScreen) && k <= (hook(kHookFlatScreenFail) ? kGemmMaxK : kScreenMaxK);
}
// Whether the threshold sample of a chunk (sample_thresholds) runs on the persistent tile too (flat_gemm_sample_big_kernel: the
// screen's operands, one product q_hi.x_hi) instead of the fp32 128 x 128 tile: exactly where the chunk nominates on the split
// tile (gemm_runs_split's answer, with or without the screen) and has a sample.  The ONE place that decides.  The sampled scores
// need no error bound and no margin follows them (screen_gemm_eps, split_gemm_eps are untouched): they only CHOOSE a threshold.
// Whatever it is, the nomination GEMM appends every row ITS score puts below it and the proofs argue from that threshold and that
// GEMM's margin; on these paths gemm_skips_sample() is false, so no sampled score becomes an appended key.  A threshold a
// little off costs time only: too low, a proof fails and the retry or the exhaustive kernel answers; too high, longer lists
// (vg_index_flat_appended shows both).  Values bfloat16 cannot hold: a row with |x| >= 2^128 (1 - 2^-9), an Inf or a NaN makes
// sample scores Inf or NaN (the fp32 sample: the same for Inf and NaN, finite or Inf for the first).  flat_select_kernel and
// topk_merge_kernel order scores by make_key's bits, as they do today: a NaN with the sign bit sorts below -Inf, one without above
// +Inf, so a NaN may become a threshold; flat_thr_cap_kernel replaces a NaN or an Inf by its bound, and where the bound itself is
// not finite the tile's +-1e30 clamp stands in.  Such a row has |x|^2 = Inf or NaN: d_norm_max is not finite, no proof holds, and
// the exhaustive kernel or the heap replay answers as before this kernel.
// (test hook kHookFlatF32Sample: the fp32 128 x 128 sample as before)
static bool sample_runs_big(bool split, bool use_sample)
{
    return split && use_sample && !hook(kHookFlatF32Sample);
}
constexpr int kScanMaxBatch = 4;  // ... and the batch size up to which the scan beats the 32-query GEMM tile
template <bool DOT>
__global__ __launch_bounds__(256) void flat_scan_mq_kernel(const float *__restrict__ base, int64_t n, int dim,
                                                           const float *__restrict__ queries, int nq, int slices,
                                                           int k, uint64_t *__restrict__ partial)
{
    extern __shared__ float qlds[];  // nq * dim floats, then the merge scratch
    uint64_t *lists = reinterpret_cast<uint64_t *>(qlds + static_cast<size_t>(kScanQB) * dim);
    int *valid = reinterpret_cast<int *>(lists + 4 * 64);
    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < nq * dim; t += 256) qlds[t] = queries[t];
    __syncthreads();
    const Sub16 sub = Sub16::make(tid);
    const int nblk = dim >> 6;
    const int64_t r0 = n * s / slices, r1 = n * (s + 1) / slices;
    WaveTopK tk[kScanQB];
#pragma unroll
    for (int qi = 0; qi < kScanQB; qi++) tk[qi].init(k);
    for (int64_t i0 = r0 + wave * 4; i0 < r1; i0 += 16) {
        const int64_t i = i0 + (lane >> 4);
        const bool live = i < r1;
        const float *row = base + (live ? i : r1 - 1) * dim;
        float4 rr[16];
        const float4 *r4 = reinterpret_cast<const float4 *>(row) + sub.f4;
#pragma unroll
        for (int e = 0; e < 16; e++)
            if (e < nblk) rr[e] = load_stream(r4 + e * 16);
#pragma unroll
        for (int qi = 0; qi < kScanQB; qi++) {
            if (qi < nq) {
                const float v = exact_rowregs16<DOT>(rr, nblk, row, qlds + static_cast<size_t>(qi) * dim, dim, sub);
                uint64_t key = kKeyMax;
                if (live && (lane & 15) == 0) key = make_key(v, static_cast<uint32_t>(i), DOT);
                tk[qi].offer(key, lane);
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < kScanQB; qi++) {
        if (qi < nq) {
            wg_rank_merge<4>(tk[qi], lists, valid, wave, lane, tid, k,
                             partial + (static_cast<int64_t>(qi) * slices + s) * k);
            __syncthreads();
        }
    }
}

// overwrite the results of the fallback queries from the exact scan's merged lists
__global__ void flat_patch_kernel(const int *__restrict__ fallback, const int *__restrict__ always, int k,
                                  const uint32_t *__restrict__ fids, const float *__restrict__ fscores,
                                  uint32_t *__restrict__ ids, float *__restrict__ scores)
{
    const int64_t q = blockIdx.x;
    if (!(always && always[0]) && !fallback[q]) return;
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        ids[q * k + i] = fids[q * k + i];
        scores[q * k + i] = fscores[q * k + i];
    }
}

// page `off / 64` of a paged exhaustive result (k > 64): kk results per flagged query land at ids[q*k + off ..),
// and the last key of the page becomes the floor of the next one (kKeyMax when the rows ran out)
__global__ void flat_page_patch_kernel(const int *__restrict__ fallback, const int *__restrict__ always, int k, int off,
                                       int kk, bool descending, const uint32_t *__restrict__ fids,
                                       const float *__restrict__ fscores, uint32_t *__restrict__ ids,
                                       float *__restrict__ scores, uint64_t *__restrict__ min_keys)
{
    const int64_t q = blockIdx.x;
    if (!(always && always[0]) && !(fallback && fallback[q])) return;
    for (int i = threadIdx.x; i < kk; i += blockDim.x) {
        ids[q * k + off + i] = fids[q * kk + i];
        scores[q * k + off + i] = fscores[q * kk + i];
    }
    if (threadIdx.x == 0) {
        const uint32_t last = fids[q * kk + kk - 1];
        min_keys[q] = last == VG_INVALID_ID ? kKeyMax : make_key(fscores[q * kk + kk - 1], last, descending);
    }
}

// all queries of a paged scan (k > 64 through a kernel that keeps 64 keys per wave): copy page `off / 64` and
// make its last key the floor of the next page
int32_t launch_page_patch(int64_t nq, int k, int off, int kk, bool descending, const int *always_one,
                          const uint32_t *fids, const float *fscores, uint32_t *ids, float *scores, uint64_t *min_keys,
                          hipStream_t st)
{
    VG_LAUNCH(flat_page_patch_kernel, dim3(static_cast<unsigned>(nq)), dim3(64), 0, st, nullptr, always_one, k, off, kk,
              descending, fids, fscores, ids, scores, min_keys);
    return VG_OK;
}

// ---- the host side of a nomination: each step once --------------------------------------------------------------------------
// The operands of a nomination on the fp32 rows (LDS-DMA, where the caller has it: rows of whole float4, 16-byte aligned)
static GemmOperands fp32_operands(const vg_index *idx, const float *queries, bool dma = true)
{
    return {queries, idx->d_vectors, idx->n, idx->dim, idx->d_norms, false, dma && idx->dim % 4 == 0 && aligned16(queries) && aligned16(idx->d_vectors)};
}
// The operands of a nomination on a bfloat16 image of the n rows (rows_bf16: dim_pad bfloat16 a row, `norms` its norms): the
// queries rounded and padded alike into qbf — one launch — and the image.
// (scale, or null: the queries multiplied by it element by element first — f32_scaled_to_bf16_pad_kernel)
static int32_t gemm_operands(const float *queries, int64_t cnt, int dim, int64_t n, const float *norms, const uint16_t *rows_bf16, int dim_pad,
                             uint16_t *qbf, hipStream_t st, GemmOperands *ops, const float *scale = nullptr)
{
    const dim3 grid(static_cast<unsigned>((cnt * dim_pad + 255) / 256));
    if (scale)
        VG_LAUNCH(f32_scaled_to_bf16_pad_kernel, grid, dim3(256), 0, st, queries, scale, cnt, dim, dim_pad, qbf);
    else
        VG_LAUNCH(f32_to_bf16_pad_kernel, grid, dim3(256), 0, st, queries, cnt, dim, dim_pad, qbf);
    *ops = {reinterpret_cast<const float *>(qbf), reinterpret_cast<const float *>(rows_bf16), n, dim_pad / 2, norms, true, true};
    return VG_OK;
}
// the columns of a row sample: every stride-th 128-row tile of n rows, whole tiles
static int64_t sample_cols(int64_t n, int stride)
{
    const int64_t nt = (n + kGemmBN - 1) / kGemmBN;
    return (nt + stride - 1) / stride * kGemmBN;
}
// the slices flat_select_kernel cuts a query's cols scores into: per_slice scores each, at most `most`
static int select_slices(int64_t cols, int per_slice, int most)
{
    return static_cast<int>(std::min<int64_t>(most, std::max<int64_t>(1, cols / per_slice)));
}
constexpr int kFlatKc = 64;  // nominated candidates per query
// Scratch of a nomination of cnt queries: the threshold step's (the sampled scores sc[cnt][cols], the select's lists, the merge's
// row ids) and what it produces (nom: the thresholds, the counts, cap appended keys a query, the 64 picked).  What it was sized
// with is what it is launched with.  A driver's scratch derives from it and carves itself where it is constructed, from `base` —
// null: it only measures — and `bytes` is what it takes.
struct NomScratch {
    float *sc;
    uint64_t *partial;
    uint32_t *sid;
    int64_t cols;
    int slices;  // (slices_ = 0: the flat searches' rule)
    ProbeNominated nom;
    size_t bytes;
    void carve(Carve &c, int64_t cnt, int64_t cols_, int sel_k, int cap, bool sampled = true, int slices_ = 0)
    {
        cols = cols_;
        slices = slices_ ? slices_ : select_slices(cols, 4096, 64);
        nom.sel_k = sel_k;
        nom.cap = cap;
        c.take(sc, sampled ? cnt * cols : 1);  // (not sampled: no launch reads it)
        c.take(partial, cnt * slices * sel_k);
        c.take(sid, cnt * sel_k);
        c.take(nom.thr, cnt * sel_k);
        c.take(nom.counts, cnt);
        c.take(nom.cand, cnt * cap);
        c.take(nom.cand_id, cnt * kFlatKc);
        c.take(nom.cand_sc, cnt * kFlatKc);
    }
};
static int32_t launch_flat_select(const NomScratch &s, int64_t cnt, int sel_k, hipStream_t st)
{
    VG_LAUNCH(flat_select_kernel, dim3(s.slices, static_cast<unsigned>(cnt)), dim3(kSelThreads), 0, st, s.sc, s.cols, s.slices, sel_k, s.partial);
    return VG_OK;
}
// per query the sel_k best of its scores s.sc, ascending, into thr[cnt][sel_k] (ids: their columns)
static int32_t select_thresholds(const NomScratch &s, int64_t cnt, int sel_k, uint32_t *ids, float *thr, hipStream_t st)
{
    VG_TRY(launch_flat_select(s, cnt, sel_k, st));
    return launch_topk_merge(s.partial, cnt, s.slices, sel_k, false, ids, thr, st);
}
// (a) of a nomination: a query's thresholds are the sel_k best scores of a row sample (every stride-th row tile; rows its filter
// rejects score +Inf), the last of them its append threshold; not `sampled` (few rows: the list holds them all): +Inf
// (image: the sample on the persistent tile, from flat_split_queries_kernel's compact hi-only image of the queries, one workgroup on each of
// the `cus` compute units — sample_runs_big)
static int32_t sample_thresholds(const NomCall &c, const NomScratch &s, int stride, int sel_k, float *thr, bool sampled, const uint32_t *image = nullptr,
                                 int cus = 0)
{
    if (!sampled) {
        VG_LAUNCH(fill_f32_kernel, dim3(static_cast<unsigned>((c.cnt * sel_k + 255) / 256)), dim3(256), 0, c.st, thr, c.cnt * sel_k, INFINITY);
        return VG_OK;
    }
    GemmArgs a = GemmArgs::sample(c, s.sc, stride, s.cols);
    if (image) a.sample_tile(image).wide(nullptr, cus);
    VG_TRY(launch_gemm<1>(a));
    return select_thresholds(s, c.cnt, sel_k, s.sid, thr, c.st);
}
static int32_t launch_flat_pick(const ProbeNominated &nom, int64_t cnt, const int *only, hipStream_t st)
{
    VG_LAUNCH(flat_pick_kernel, dim3(static_cast<unsigned>(cnt)), dim3(256), 0, st, nom.cand, nom.counts, nom.cap, kFlatKc, nom.cand_id, nom.cand_sc, only);
    return VG_OK;
}
// (d) of a nomination on the fp32 rows: the exact re-score and the proof, ids / scores [cnt][k] and fail[q] = 1 where the proof
// does not hold.  k > 64: every appended row, sorted in LDS; k > kGemmMaxK: every appended row; otherwise the kFlatKc picked ones
// (nom.thr null: the unfused variant's 64 best of the score matrix; only: see flat_verify_kernel).
static int32_t launch_flat_verify(bool dot, int k, const vg_index *idx, const float *queries, int64_t cnt, const ProbeNominated &nom,
                                  float eps_extra, uint32_t *ids, float *scores, int *fail, const int *only, hipStream_t st)
{
    return with_metric(dot, [&](auto dot_c) -> int32_t {
        constexpr bool DOT = decltype(dot_c)::value;
        const dim3 grid(static_cast<unsigned>(cnt)), threads(256);
        if (nom.thr && k > 64)
            VG_LAUNCH(flat_verify_sort_kernel<DOT>, grid, threads, sizeof(uint64_t) * static_cast<size_t>(nom.cap), st, idx->d_vectors, idx->dim, queries,
                      idx->d_norm_max, nom.cand, nom.counts, nom.cap, k, ids, scores, fail, nom.thr, nom.sel_k, nom.sel_k - 1, eps_extra);
        else if (nom.thr && k > kGemmMaxK)
            VG_LAUNCH(flat_verify_all_kernel<DOT>, grid, threads, 0, st, idx->d_vectors, idx->dim, queries, idx->d_norm_max, nom.cand, nom.counts,
                      nom.cap, k, ids, scores, fail, nom.thr, nom.sel_k, nom.sel_k - 1, eps_extra);
        else
            VG_LAUNCH(flat_verify_kernel<DOT>, grid, threads, 0, st, idx->d_vectors, idx->n, idx->dim, queries, idx->d_norm_max, nom.cand_id,
                      nom.cand_sc, kFlatKc, k, ids, scores, fail, nom.thr, nom.sel_k, nom.sel_k - 1, nom.counts, nom.cap, eps_extra, only);
        return VG_OK;
    });
}

// ---- vg_search_flat -----------------------------------------------------------------------------------------------------------
// One call, or one chunk of it (range): device pointers; mask: see flat_search_masked
struct FlatCall {
    vg_index *idx;
    int k;
    hipStream_t st;
    bool dot;
    const float *q;
    int64_t nq;
    const uint8_t *mask;
    int64_t mask_stride;
    uint32_t *oid;
    float *osc;
    int64_t n = idx->n;
    int dim = idx->dim;
    // queries q0 .. q0 + cnt - 1 with their filters and results: the offsets of a chunk, in one place
    FlatCall range(int64_t q0, int64_t cnt) const
    {
        FlatCall r = *this;
        r.q += q0 * dim, r.nq = cnt, r.oid += q0 * k, r.osc += q0 * k;
        if (mask) r.mask += q0 * mask_stride;
        return r;
    }
    // its nomination on the fp32 rows (test hook kHookFlatNoDma: force the register-staged GEMM)
    NomCall nom() const { return {st, dot, fp32_operands(idx, q, !hook(kHookFlatNoDma)), nq, mask, mask_stride}; }
};
constexpr int kFlatCap = 4096;         // candidate keys per query (fused path, and the nomination on a quantizer's image)
constexpr int kFlatSampleStride = 64;  // every 64th 128-row tile is sampled
static int exact_slices(int64_t n) { return static_cast<int>(std::min<int64_t>(256, std::max<int64_t>(1, n / 64))); }
// The sizes of the GEMM paths, fixed per call, and their scratch for qc queries, shared by the chunks
struct FlatScratch : NomScratch {
    bool fused;       // (test hook kHookFlatUnfused: materialise the score matrix)
    bool use_sample;  // n <= cap: threshold +Inf, every row is appended
    bool bf16;        // the bfloat16 filter (bf16_filter_eps)
    bool may_split;   // a chunk above 128 queries may nominate on the split tile (gemm_runs_split, decided per chunk)
    int ex_slices, pk;  // the exhaustive fall-back: slices of the rows, results per page
    int64_t qc;       // queries per chunk
    int *flags, *todo;  // the proofs' verdicts (flags[qc]: flat_todo_kernel's "every query" switch) and step 4's work list
    uint64_t *fpartial, *min_keys;
    uint32_t *fid;
    float *fsc;
    uint16_t *qbf;  // the chunk's queries in bfloat16, or as the split tile's hi | lo image
    uint32_t *qhi;  // beside the hi | lo image: the compact hi-only one of the screen and the sample (whole 256-query tiles)
    int *counts_wide;
    uint32_t *tile_active;  // the retry's query tiles (flat_retry_prepare_kernel)
    FlatScratch(const FlatCall &c, bool unfused, char *base) : fused(!unfused), use_sample(fused && c.n > kFlatCap)
    {
        // (any dim: the copies' rows are padded with zeros to whole K steps, vectors_bf16_dim)
        bf16 = c.idx->d_vectors_bf16 != nullptr && fused && !hook(kHookFlatNoDma);
        // thresholds kept per query: the sample_j-th best score of the row sample is the query's, ~64 * sample_j rows pass it
        // (k > 64: ~3k of them); the unfused variant: the 64 nominated candidates
        const int sel_k = !fused ? kFlatKc : c.k <= 64 ? 8 : std::min(64, std::max(8, (3 * c.k + 63) / 64));
        ex_slices = exact_slices(c.n);
        pk = std::min(c.k, 64);
        // query chunk: whole 128-query tiles; unfused keeps the score matrix <= 2 GiB
        qc = fused ? 4096 : (int64_t(2) << 30) / (c.n * 4);
        if (qc > 4096) qc = 4096;
        if (qc >= kGemmBM) qc = (qc / kGemmBM) * kGemmBM;
        if (qc < 1) qc = 1;
        if (qc > c.nq) qc = c.nq;
        // without the filter, a chunk above 128 queries nominates on the split tile (gemm_runs_split, decided per chunk: the
        // margin grows by split_gemm_eps, the chunk's queries are written as a hi | lo image, the appends count in wide counters)
        may_split = gemm_runs_split(fused, bf16, true, qc, c.dim, kFlatCap, sel_k);
        Carve cv{base};
        // (unfused: nothing is appended, cap 0 — flat_verify_kernel reads no cap where it has no threshold)
        carve(cv, qc, fused ? sample_cols(c.n, kFlatSampleStride) : c.n, sel_k, fused ? kFlatCap : 0, !fused || use_sample);
        cv.take(flags, qc + 1);
        cv.take(todo, qc + 1);
        cv.take(fpartial, qc * ex_slices * pk);
        cv.take(fid, qc * pk);
        cv.take(fsc, qc * pk);
        cv.take(min_keys, qc);
        cv.take(qbf, bf16 ? qc * c.idx->vectors_bf16_dim : may_split ? 2 * qc * c.dim : 0);
        cv.take(qhi, may_split ? flat_hi_image_rows(qc) * (c.dim / 2) : 0);
        cv.take(counts_wide, bf16 || may_split ? qc * kCountLine : 0);
        cv.take(tile_active, may_split ? 1 : 0);
        bytes = cv.off;
    }
};

// small batch: HBM-bound exact scan, kScanQB queries per pass over the rows
static int32_t flat_scan_small(const FlatCall &c)
{
    const int slices = static_cast<int>(std::min<int64_t>(4 * c.idx->ctx->compute_units, std::max<int64_t>(1, c.n / 64)));
    ArenaCall ar(c.idx->ctx, c.st);
    const int i_partial = ar.add(sizeof(uint64_t) * static_cast<size_t>(c.nq) * slices * c.k);
    VG_TRY(ar.commit());
    uint64_t *partial = ar.get<uint64_t>(i_partial);
    const size_t lds = sizeof(float) * static_cast<size_t>(kScanQB) * c.dim + 4 * 64 * sizeof(uint64_t) + 64;
    for (int64_t q0 = 0; q0 < c.nq; q0 += kScanQB) {
        const int cnt = static_cast<int>(std::min<int64_t>(kScanQB, c.nq - q0));
        ProfScope prof(c.idx->ctx, "flat_scan", c.st);
        auto kern = c.dot ? flat_scan_mq_kernel<true> : flat_scan_mq_kernel<false>;
        VG_LAUNCH(kern, dim3(slices), dim3(256), lds, c.st, c.idx->d_vectors, c.n, c.dim, c.q + q0 * c.dim, cnt, slices, c.k, partial + q0 * slices * c.k);
    }
    VG_TRY(launch_topk_merge(partial, c.nq, slices, c.k, c.dot, c.oid, c.osc, c.st));
    return launch_flat_todo(nullptr, nullptr, static_cast<int>(c.nq), nullptr, c.idx->d_flat_stats, c.st);
}

// step 4: the exhaustive exact kernel for the chunk's queries of the work list, kk results each after floor_keys (null: the best)
static int32_t launch_flat_exact(const FlatCall &c, const int *todo, int ex_slices, int kk, uint64_t *fpartial, const uint64_t *floor_keys)
{
    const unsigned slots = static_cast<unsigned>(std::min<int64_t>(c.nq, kExactSlots));
    auto kern = c.dot ? flat_exact_kernel<true> : flat_exact_kernel<false>;
    VG_LAUNCH(kern, dim3(ex_slices, slots), dim3(256), 0, c.st, c.idx->d_vectors, c.n, c.dim, c.q, todo, ex_slices, kk, fpartial, floor_keys, c.mask,
              c.mask_stride);
    return VG_OK;
}
// kGemmMaxK < k <= 64 of the unfused variant (64 nominated candidates cannot prove k near 64): the exhaustive exact kernel for
// every query, one pass over the rows per query
static int32_t flat_exact_every_query(const FlatCall &call)
{
    const int ex_slices = exact_slices(call.n);
    const int64_t qc = std::min<int64_t>(call.nq, 4096);
    ArenaCall ar(call.idx->ctx, call.st);
    const int i_flags = ar.add(sizeof(int) * (static_cast<size_t>(qc) + 1));
    const int i_todo = ar.add(sizeof(int) * (static_cast<size_t>(qc) + 1));
    const int i_fpartial = ar.add(sizeof(uint64_t) * static_cast<size_t>(qc) * ex_slices * call.k);
    VG_TRY(ar.commit());
    int *flags = ar.get<int>(i_flags), *todo = ar.get<int>(i_todo);
    uint64_t *fpartial = ar.get<uint64_t>(i_fpartial);
    VG_HIP(hipMemsetAsync(flags, 0, sizeof(int) * static_cast<size_t>(qc), call.st));
    VG_HIP(hipMemsetAsync(flags + qc, 1, sizeof(int), call.st));  // "every query" switch of flat_todo_kernel
    for (int64_t q0 = 0; q0 < call.nq; q0 += qc) {
        const FlatCall c = call.range(q0, std::min(qc, call.nq - q0));
        VG_TRY(launch_flat_todo(flags, flags + qc, static_cast<int>(c.nq), todo, c.idx->d_flat_stats, c.st));
        VG_TRY(launch_flat_exact(c, todo, ex_slices, c.k, fpartial, nullptr));
        VG_TRY(launch_topk_merge(fpartial, c.nq, ex_slices, c.k, c.dot, c.oid, c.osc, c.st));
    }
    return VG_OK;
}

// The unfused variant (test hook) of a chunk: its whole score matrix, the 64 best per query, their re-score and proof
static int32_t flat_unfused_chunk(const FlatCall &c, const FlatScratch &s)
{
    const NomCall nc = c.nom();
    {
        ProfScope prof(c.idx->ctx, "flat_gemm", c.st);
        VG_TRY(launch_gemm<0>(GemmArgs::sample(nc, s.sc, 1, c.n)));
    }
    {
        ProfScope prof(c.idx->ctx, "flat_select", c.st);
        VG_TRY(launch_flat_select(s, c.nq, kFlatKc, c.st));
    }
    VG_TRY(launch_topk_merge(s.partial, c.nq, s.slices, kFlatKc, false, s.nom.cand_id, s.nom.cand_sc, c.st));
    ProbeNominated nom = s.nom;
    nom.thr = nullptr;  // nothing was appended: the proof argues from the 64th best score
    return launch_flat_verify(c.dot, c.k, c.idx, c.q, c.nq, nom, 0.0f, c.oid, c.osc, s.flags, nullptr, c.st);
}

// The retry behind a screen.  A query whose proof held is finished; for the others (normally none) the split tile
// runs on the 256-query tiles that hold one — launched ALWAYS, once per chunk: with no tile marked every workgroup
// returns at once — then the pick and the proof again, for the flagged queries only and with the split tile's margin.
// (test hook kHookFlatScreenFail: every screen proof counts as failed)
static int32_t flat_screen_retry(const FlatCall &c, const NomCall &nc, const FlatScratch &s)
{
    const ProbeNominated &nom = s.nom;
    VG_LAUNCH(flat_retry_prepare_kernel, dim3(1), dim3(kBigBM), 0, c.st, s.flags, hook(kHookFlatScreenFail), static_cast<int>(c.nq), nom.thr,
              nom.sel_k, nom.sel_k - 1, nom.counts, s.counts_wide, s.tile_active, c.idx->d_flat_stats);
    {
        ProfScope prof(c.idx->ctx, "flat_retry", c.st);
        VG_TRY(launch_gemm<2>(GemmArgs::append(nc, nom.thr, nom.sel_k, nom.counts, nom.cand, nom.cap)
                                  .wide(s.counts_wide, c.idx->ctx->compute_units)
                                  .split_tile(reinterpret_cast<const uint32_t *>(s.qbf))
                                  .retry(s.tile_active)));
    }
    VG_TRY(launch_flat_pick(nom, c.nq, s.flags, c.st));
    return launch_flat_verify(c.dot, c.k, c.idx, c.q, c.nq, nom, split_gemm_eps(c.dot, c.dim), c.oid, c.osc, s.flags, s.flags, c.st);
}

// The fused path of a chunk: thresholds from a row sample, the GEMM appending what falls below them, the re-score and the proof
static int32_t flat_fused_chunk(const FlatCall &c, const FlatScratch &s)
{
    const vg_index *idx = c.idx;
    const ProbeNominated &nom = s.nom;
    NomCall nc = c.nom();
    const bool split = gemm_runs_split(true, s.bf16, nc.ops.dma, c.nq, c.dim, nom.cap, nom.sel_k);
    // ... behind a screen: the hi halves' product and the wide margin first, the split tile for the queries that leaves open
    const bool screen = gemm_runs_screen(split, c.k);
    const float eps_extra = screen ? screen_gemm_eps(c.dot, c.dim) : split ? split_gemm_eps(c.dot, c.dim) : s.bf16 ? bf16_filter_eps(c.dot) : 0.0f;
    if (s.bf16) VG_TRY(gemm_operands(c.q, c.nq, c.dim, c.n, idx->d_norms, idx->d_vectors_bf16, idx->vectors_bf16_dim, s.qbf, c.st, &nc.ops));
    // (the images of the queries first, one launch: hi | lo for the split tile — the nomination without a screen, the retry behind
    // one — and the compact hi-only one for the screen and, where sample_runs_big() says so, the sample)
    if (split)
        VG_LAUNCH(flat_split_queries_kernel, dim3(static_cast<unsigned>((flat_hi_image_rows(c.nq) * (c.dim / 2) + 255) / 256)), dim3(256), 0, c.st, c.q,
                  c.nq, c.dim, reinterpret_cast<uint32_t *>(s.qbf), s.qhi);
    // (a) threshold per query from a row sample
    VG_TRY(sample_thresholds(nc, s, kFlatSampleStride, nom.sel_k, nom.thr, s.use_sample, sample_runs_big(split, s.use_sample) ? s.qhi : nullptr,
                             idx->ctx->compute_units));
    if (s.bf16 || split) VG_LAUNCH(flat_thr_cap_kernel, dim3(nc.ucnt()), dim3(64), 0, c.st, nom.thr, nom.sel_k, c.q, c.dim, idx->d_norm_max);
    // (b) the GEMM, appending every element below its query's threshold.  The sampled tiles' scores are in `sc` already,
    // bit for bit, where (a) ran the same tile: what passes there is appended from `sc` (which also sets the counters)
    // and the GEMM leaves those tiles out — 63/64 of the elements (test hook kHookFlatRescoreSample: all of them again)
    const bool once = s.use_sample && gemm_skips_sample(nc.ops.dma, c.nq, s.bf16, split);
    if (!once) VG_HIP(hipMemsetAsync(nom.counts, 0, sizeof(int) * static_cast<size_t>(c.nq), c.st));
    {
        ProfScope prof(idx->ctx, "flat_gemm", c.st);
        if (once)
            VG_LAUNCH(flat_sample_append_kernel, dim3(nc.ucnt()), dim3(kSampleAppendThreads), 0, c.st, s.sc, s.cols, kFlatSampleStride, nom.thr,
                      nom.sel_k, nom.sel_k - 1, nom.counts, nom.cand, nom.cap);
        GemmArgs a = GemmArgs::append(nc, nom.thr, nom.sel_k, nom.counts, nom.cand, nom.cap);
        a.wide(s.bf16 || split ? s.counts_wide : nullptr, idx->ctx->compute_units).skipping(once ? kFlatSampleStride : 0);
        if (screen)
            a.screen_tile(s.qhi);
        else if (split)
            a.split_tile(reinterpret_cast<const uint32_t *>(s.qbf));
        VG_TRY(launch_gemm<2>(a));
    }
    // (c) the kc best appended keys (k > kGemmMaxK: all of them go to the exact re-score), (d) the re-score and the proof
    if (c.k <= kGemmMaxK) VG_TRY(launch_flat_pick(nom, c.nq, nullptr, c.st));
    VG_TRY(launch_flat_verify(c.dot, c.k, idx, c.q, c.nq, nom, eps_extra, c.oid, c.osc, s.flags, nullptr, c.st));
    return screen ? flat_screen_retry(c, nc, s) : VG_OK;
}

// test hook kHookFlatDebug: what the proofs and lists of the chunk at query q0 came to (waits for the stream)
static void flat_debug_counts(const FlatCall &c, int64_t q0, const FlatScratch &s)
{
    std::vector<int> hf(c.nq), hc(c.nq);
    (void)hipMemcpyAsync(hf.data(), s.flags, sizeof(int) * c.nq, hipMemcpyDeviceToHost, c.st);
    (void)hipMemcpyAsync(hc.data(), s.nom.counts, sizeof(int) * c.nq, hipMemcpyDeviceToHost, c.st);
    (void)hipStreamSynchronize(c.st);
    int64_t nf = 0, csum = 0, cmax = 0;
    for (int f : hf) nf += f != 0;
    for (int n : hc) { csum += n; cmax = std::max<int64_t>(cmax, n); }
    fprintf(stderr, "[vg_search_flat] chunk q0=%lld cnt=%lld: %lld queries failed the proof; "
            "appended candidates avg %.1f max %lld\n", (long long)q0, (long long)c.nq, (long long)nf,
            s.fused ? double(csum) / c.nq : 0.0, (long long)(s.fused ? cmax : 0));
}

// step 4 always launches, on the work list the proofs left behind (normally empty).  The exhaustive kernel keeps 64 keys per
// wave: k > 64 comes in pages of 64, each page scanning for the keys after the previous page's last one
static int32_t flat_fallback_pages(const FlatCall &c, const FlatScratch &s)
{
    const int *always = s.flags + s.qc;
    const dim3 grid(static_cast<unsigned>(c.nq));
    for (int off = 0; off < c.k; off += 64) {
        const int kk = std::min(64, c.k - off);
        VG_TRY(launch_flat_exact(c, s.todo, s.ex_slices, kk, s.fpartial, off ? s.min_keys : nullptr));
        VG_TRY(launch_topk_merge(s.fpartial, c.nq, s.ex_slices, kk, c.dot, s.fid, s.fsc, c.st, s.flags, always));
        if (c.k <= 64)
            VG_LAUNCH(flat_patch_kernel, grid, dim3(64), 0, c.st, s.flags, always, c.k, s.fid, s.fsc, c.oid, c.osc);
        else
            VG_LAUNCH(flat_page_patch_kernel, grid, dim3(64), 0, c.st, s.flags, always, c.k, off, kk, c.dot, s.fid, s.fsc, c.oid, c.osc, s.min_keys);
    }
    return VG_OK;
}

// The GEMM paths: the batch in chunks of whole query tiles, each nominated and proved, its open queries scanned exhaustively
static int32_t flat_gemm_search(const FlatCall &call, bool unfused)
{
    ArenaCall ar(call.idx->ctx, call.st);
    const int i_all = ar.add(FlatScratch(call, unfused, nullptr).bytes);
    VG_TRY(ar.commit());
    const FlatScratch s(call, unfused, ar.get<char>(i_all));
    int *always = s.flags + s.qc;  // test hook kHookFlatForceExact: run step 4 for every query
    VG_HIP(hipMemsetAsync(always, hook(kHookFlatForceExact) ? 1 : 0, sizeof(int), call.st));
    for (int64_t q0 = 0; q0 < call.nq; q0 += s.qc) {
        const FlatCall c = call.range(q0, std::min(s.qc, call.nq - q0));
        VG_TRY(s.fused ? flat_fused_chunk(c, s) : flat_unfused_chunk(c, s));
        VG_TRY(launch_flat_todo(s.flags, always, static_cast<int>(c.nq), s.todo, c.idx->d_flat_stats, c.st, s.fused ? s.nom.counts : nullptr));
        if (hook(kHookFlatDebug)) flat_debug_counts(c, q0, s);
        VG_TRY(flat_fallback_pages(c, s));
    }
    return VG_OK;
}

// vg_search_flat, and — with `mask` (a DEVICE pointer: bit i of byte i/8 of query q's mask at mask + q * mask_stride,
// stride 0 = one mask) — the batched fp32 leg of vg_search_flat_filtered (k_probe.hip): the rows a query's filter rejects
// are left out of its threshold sample and of its candidate list, so the proof argues about the rows it wants only
// ("every wanted row not appended scores at or above the threshold"); the exhaustive fallback skips them too.
// l2_scores: squared-L2 scores whatever the index's metric (vg_search_hnsw_brute on a Cosine index: hnsw's distance there is
// 0.5 * squared L2, flat.Segment's is the dot product)
int32_t flat_search_masked(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask, int64_t mask_stride, uint32_t *ids,
                           float *scores, void *stream, bool l2_scores, bool cand_replay)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_search_flat: NULL index");
    VG_CHECK(nq >= 0 && k >= 0, VG_ERR_INVALID_ARG, "vg_search_flat: negative nq or k");
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    VG_CHECK(idx->n == 0 || idx->d_vectors, VG_ERR_NOT_READY, "vg_search_flat: index has no fp32 vectors");
    VG_CHECK(queries && ids && scores, VG_ERR_INVALID_ARG, "vg_search_flat: NULL buffer");
    VG_CHECK(k <= kFlatMaxK, VG_ERR_UNSUPPORTED, "vg_search_flat: k=%d exceeds %d", k, kFlatMaxK);
    // k beyond what 64 nominated candidates can prove: the fused GEMM path re-scores every appended row
    // (flat_verify_all_kernel); the unfused score-matrix variant (test hook) stops at 64
    const bool unfused = hook(kHookFlatUnfused) && mask == nullptr;
    VG_CHECK(k <= 64 || !unfused, VG_ERR_UNSUPPORTED, "vg_search_flat: k=%d needs the fused GEMM path", k);

    SearchIO io;
    VG_TRY(io.init(idx->ctx, stream, queries, static_cast<size_t>(nq) * idx->dim, ids, scores, static_cast<size_t>(nq) * k));
    const bool dot = idx->metric != VG_METRIC_L2 && !l2_scores;
    const FlatCall c{idx, k, io.st, dot, io.q.ptr, nq, mask, mask_stride, io.oid.ptr, io.osc.ptr};
    const bool scan_small = mask == nullptr && nq <= kScanMaxBatch && k <= 64 && c.dim % 4 == 0 && c.dim <= 1024 && c.dim >= 64 &&
                            !hook(kHookFlatNoScan) && !hook(kHookFlatForceExact) && !unfused && aligned16(idx->d_vectors);
    if (c.n == 0)
        VG_TRY(empty_results(nq, k, dot, c.oid, c.osc, c.st));
    else if (scan_small)
        VG_TRY(flat_scan_small(c));
    else if (unfused && k > kGemmMaxK)
        VG_TRY(flat_exact_every_query(c));
    else
        VG_TRY(flat_gemm_search(c, unfused));
    // queries whose scores may hold a NaN (a non-finite query value / row, an overflowing dot product): the reference's heap,
    // operation by operation (vg_cand_replay.hpp); every other query returns from this launch at once
    if (c.n > 0 && cand_replay)
        VG_TRY(launch_cand_replay(FlatF32Scorer{idx->d_vectors, idx->d_norm_max + 1, c.dim, dot, 0}, c.q, c.dim, c.n, nq, k, dot, mask, mask_stride,
                                  c.oid, c.osc, c.st));
    return io.finish();
}

// ---- the grouped nomination of the probed scans -------------------------------------------------------------------------------
// The nomination + proof of vg_search_flat over MANY (queries, rows) problems in one set of launches: the partition-probed search
// of k_probe.hip.  pair_queries: the (query, probe) pairs' query vectors bucketed by partition ([pairs, dim]); groups[g]: partition
// g's pairs and rows; first_block_*: each group's first workgroup in the sample / main GEMM launch (device; the totals are not
// known to the host: the grids are the host's upper bounds, surplus workgroups leave at once).  Per pair: ids / scores [pairs, k]
// = its partition's k best rows by (score, row id) with exact scores, and fail[pair] = 1 where the proof does not hold (the caller
// answers those queries with the exact probe kernels).  k <= kGemmMaxK; fp32 rows, dim % 4 == 0, 16-byte aligned.
// thresholds kept per pair: the 8th best of the 1/8 row sample passes ~64 rows — enough for the 64-candidate re-score (k <= 48);
// a larger k re-scores everything that passed and wants ~3k of them — ~5k under a bfloat16 nomination, whose proof needs the
// threshold 2^-7 (|q|^2 + |x|^2) above the k-th score: at 3k, random-normal rows of dim 768 in partitions of 8192 failed the
// proof for about every other query of 8 probes (the rank of a sampled threshold varies by 1 / sqrt(sel_k))
int probe_gemm_sel_k(int k, bool bf16) { return k <= kGemmMaxK ? 8 : std::min(64, std::max(8, ((bf16 ? 5 : 3) * k + 7) / 8)); }
// candidate keys per pair: ~64 rows fall below a pair's threshold (8th best of 1/8 of its partition); 2048 leaves 30x, and a
// batch of 65535 pairs holds 1 GiB of them (4096, the flat search's, would be 2)
constexpr int kProbeGemmCap = 2048;
// (scratch: one piece of the caller's arena — the caller holds the arena for the call — carved here; the layout in one place)
struct ProbeGemmScratch : NomScratch {
    uint16_t *qbf;  // bf16_dim > 0: the pairs' queries in bfloat16
    ProbeGemmScratch(char *base, int64_t pairs, int64_t ns_max, int k, int bf16_dim)
    {
        Carve c{base};
        carve(c, pairs, ns_max, probe_gemm_sel_k(k, bf16_dim > 0), kProbeGemmCap, true, select_slices(ns_max, 1024, 8));
        c.take(qbf, pairs * bf16_dim);
        bytes = c.off;
    }
};
size_t flat_probe_gemm_scratch_bytes(int64_t pairs, int64_t ns_max, int k, int bf16_dim)
{
    return ProbeGemmScratch(nullptr, pairs, ns_max, k, bf16_dim).bytes;
}
// One stage (MODE 1: sample, 2: append) over the groups: grid / first_block [MODE - 1] of the 128-query tiles (groups of more
// than 64 pairs), [MODE + 1] of the 64-query tiles (flat_gemm_dma32_grouped_kernel<.., 2>: a group of at most 64 pairs is one
// query tile, one workgroup per row tile, HBM-bound — a 128-query tile would spend the matrix cores on padding)
template <int MODE>
static int32_t launch_gemm_grouped(const GemmArgs &a, const GemmGroup *groups, int ngroups, const int64_t grid[4],
                                   const int64_t *const first_block[4], const int64_t *mask_off)
{
    const NomCall &c = a.c;
    return with_metric(c.dot, [&](auto dot_c) -> int32_t {
        constexpr bool DOT = decltype(dot_c)::value;
        const bool bf16 = c.ops.bf16;
        auto launch = [&](auto kern, size_t lds, int at) -> int32_t {
            return launch_lds(kern, dim3(static_cast<unsigned>(grid[at])), dim3(kGemmThreads), lds, c.st, groups, first_block[at], ngroups, a.queries,
                              c.ops.b, c.ops.dim_words, c.ops.norms, a.scores, a.tile_stride, a.out_cols, a.thr, a.thr_stride, a.thr_off, a.counts, a.cand, a.cap,
                              c.mask, mask_off);
        };
        VG_TRY(launch(bf16 ? flat_gemm_dma_grouped_kernel<DOT, MODE, true> : flat_gemm_dma_grouped_kernel<DOT, MODE>, kDmaLdsBytes, MODE - 1));
        return launch(bf16 ? flat_gemm_dma32_grouped_kernel<DOT, MODE, kProbeRB, true> : flat_gemm_dma32_grouped_kernel<DOT, MODE, kProbeRB>,
                      g32_lds_bytes<kProbeRB>(), MODE + 1);
    });
}

int32_t flat_probe_gemm(vg_index *idx, const float *pair_queries, int64_t pairs, const GemmGroup *groups, const int64_t *const first_block[4],
                        int ngroups, const int64_t grid[4], int sample_stride, int64_t ns_max, int k, uint32_t *pair_ids,
                        float *pair_scores, int *fail, char *scratch, const uint8_t *mask /* the batch's row filters, or null */,
                        const int64_t *mask_off /* [pairs]: byte offset of each bucketed pair's filter in `mask` */, hipStream_t st,
                        const NomImage &img, ProbeNominated *nominated)
{
    // img.rows != null: nominate on that bfloat16 row image (with its norms) instead of the fp32 rows, and leave the exact
    // re-score + proof to the caller: *nominated = where the per-pair thresholds / counts / 64 candidates are (the partition-probed
    // SQ8 scan, k_sq8_scan.hip)
    // (img.rows == idx->d_vectors_bf16: the fp32 rows' own bf16 filter, vg_index_enable_bf16_filter — the nomination runs on it,
    // the re-score and the proof below stay, the proof's margin widened as in vg_search_flat)
    const bool dot = idx->metric != VG_METRIC_L2;
    const bool bf16 = img.rows != nullptr, own_filter = bf16 && img.rows == idx->d_vectors_bf16;
    const ProbeGemmScratch s(scratch, pairs, ns_max, k, img.dim_pad);
    const ProbeNominated &nom = s.nom;
    NomCall nc{st, dot, fp32_operands(idx, pair_queries), pairs, mask, 0};
    if (bf16) VG_TRY(gemm_operands(pair_queries, pairs, idx->dim, idx->n, img.norms, img.rows, img.dim_pad, s.qbf, st, &nc.ops));
    // (a) a threshold per pair: the sel_k-th best score of every sample_stride-th row tile of its partition (columns no tile
    // writes — smaller partitions — hold +Inf)
    VG_LAUNCH(fill_f32_kernel, dim3(static_cast<unsigned>((pairs * ns_max + 255) / 256)), dim3(256), 0, st, s.sc, pairs * ns_max, INFINITY);
    VG_TRY(launch_gemm_grouped<1>(GemmArgs::sample(nc, s.sc, sample_stride, ns_max), groups, ngroups, grid, first_block, mask_off));
    VG_TRY(select_thresholds(s, pairs, nom.sel_k, s.sid, nom.thr, st));
    // (b) every element below its pair's threshold is appended to the pair's candidates
    VG_HIP(hipMemsetAsync(nom.counts, 0, sizeof(int) * static_cast<size_t>(pairs), st));
    {
        ProfScope prof(idx->ctx, "flat_probe_gemm", st);
        VG_TRY(launch_gemm_grouped<2>(GemmArgs::append(nc, nom.thr, nom.sel_k, nom.counts, nom.cand, nom.cap), groups, ngroups, grid, first_block,
                                      mask_off));
    }
    // (c) the kc best of them, (d) re-scored exactly, the k best, and the proof against everything not nominated
    // (k > kGemmMaxK: every appended row is re-scored — flat_verify_all / _sort, as in vg_search_flat)
    if (k <= kGemmMaxK) VG_TRY(launch_flat_pick(nom, pairs, nullptr, st));
    if (bf16 && !own_filter) {
        *nominated = nom;
        return VG_OK;
    }
    return launch_flat_verify(dot, k, idx, pair_queries, pairs, nom, own_filter ? bf16_filter_eps(dot) : 0.0f, pair_ids, pair_scores, fail, nullptr, st);
}

// ---- the nomination on a quantizer's bfloat16 image ---------------------------------------------------------------------------
// The nomination stage of the fused flat search over ANY bfloat16 row image with its norms: thresholds from a row sample, the
// bf16 MFMA GEMM appending what falls below them, the kc best per query — for a caller that re-scores and proves with its own
// exact distance (nominated_pass, vg_nominate.hpp: rows = a quantizer's decoded rows rounded to bfloat16, norms = |x^|^2).
// queries: cnt x idx->dim fp32 (device), cnt <= 4096; img: idx->n rows of img.dim_pad (dim rounded up to a multiple of 64, the tail
// zeros).  dot: scores are -q.x (the largest dot products first); mask: a row filter per query (mask + q * mask_stride) or for the
// batch (stride 0) — rejected rows are left out of the sample and of the candidates, as in flat_search_masked.
// *nom (all of it in `scratch`): nominate_sel_k(k) thresholds per query (the last is the query's: ~64 * sel_k rows pass it), the
// counts, every appended key, and — k <= kNomPickMaxK — the 64 best appended rows, ascending.
// The PQ nomination from the codes (img.from_codes: vg_index_enable_pq_nomination_from_codes, k_pq_nominate.hip; L2, unfiltered) has no
// image of the decoded rows: the append GEMM gathers its row tiles from the decoded codebook by the codes
// (flat_gemm_codes_big_kernel); the threshold sample needs decoded rows for every 64th 128-row tile only — those are decoded into
// the CALL's scratch (rows / 64 of the image: 1.6 % of it), their norms gathered beside them, and the sample kernels run over that
// compact image with tile stride 1: the same kernels on the same operands as the image's sample, so the same thresholds.
// thread per (compact row, granule): compact row c = sampled tile c / 128, its row c % 128
__global__ void pq_sample_rows_kernel(const uint8_t *__restrict__ codes, int64_t n, int m, const uint4 *__restrict__ cb16, int granules,
                                      const float *__restrict__ norms, int64_t rows_c, int stride, uint4 *__restrict__ out,
                                      float *__restrict__ norms_c)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t c = t / granules;
    const int j = static_cast<int>(t - c * granules);
    if (c >= rows_c) return;
    const int64_t row = (c / kGemmBN) * stride * kGemmBN + (c % kGemmBN);  // (< n: rows_c counts the sampled rows that exist)
    const int code = j < m ? codes[row * m + j] : 0;
    out[c * granules + j] = cb16[static_cast<int64_t>(j) * 256 + code];
    if (j == 0) norms_c[c] = norms[row];
}
// The SQ8 nomination from the codes (img.scale: vg_index_enable_sq8_nomination_from_codes, k_sq8_scan.hip; L2 and Dot, unfiltered)
// likewise: the queries' image is bf16(q_d inv_d), the append GEMM converts its row tiles from the code tiles
// (flat_gemm_sq8_big_kernel), and the sampled tiles are converted here the same way — bf16(code - 128), exact — so that sample and
// append score in one space, s' = |x^|^2 - 2 (q o inv).(c - 128) (Dot: -(q o inv).(c - 128)), and the thresholds need no shift.
// thread per (compact row, 16-dimension group of dim_pad / 16); groups from `groups` on are zeros
__global__ void sq8_sample_rows_kernel(const uint4 *__restrict__ tiles, int groups, int groups_pad, const float *__restrict__ norms, int64_t rows_c,
                                       int stride, uint4 *__restrict__ out, float *__restrict__ norms_c)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t c = t / groups_pad;
    const int g = static_cast<int>(t - c * groups_pad);
    if (c >= rows_c) return;
    const int64_t row = (c / kGemmBN) * stride * kGemmBN + (c % kGemmBN);  // (< n: rows_c counts the sampled rows that exist)
    uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (g < groups) {
        const uint4 code = tiles[((row >> 6) * groups + g) * 64 + (row & 63)];
        const uint32_t cw[4] = {code.x, code.y, code.z, code.w};
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const float v = static_cast<float>(static_cast<int>((cw[e >> 2] >> (8 * (e & 3))) & 0xFFu) - 128);  // (exact in bfloat16)
            w[e >> 1] |= (__float_as_uint(v) >> 16) << (16 * (e & 1));
        }
    }
    out[(c * groups_pad + g) * 2] = make_uint4(w[0], w[1], w[2], w[3]);
    out[(c * groups_pad + g) * 2 + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    if (g == 0) norms_c[c] = norms[row];
}
// the rows of every stride-th 128-row tile of n rows that exist (only the last tile of all can be short)
static int64_t sample_rows(int64_t n, int stride)
{
    const int64_t nt = (n + kGemmBN - 1) / kGemmBN, nts = (nt + stride - 1) / stride;
    const int64_t last0 = (nts - 1) * stride * kGemmBN;
    return (nts - 1) * kGemmBN + std::min<int64_t>(kGemmBN, n - last0);
}
struct NominateScratch : NomScratch {
    uint16_t *qbf;  // the queries, padded like the image's rows
    int *counts_wide;
    int64_t rows_c;   // from the codes: the sampled tiles' rows (0: an image, or too few rows for a sample) ...
    uint16_t *srows;  // ... decoded, dim_pad each ...
    float *snorms;    // ... and their norms
    NominateScratch(char *base, int64_t cnt, int64_t n, const NomImage &img, int k)
    {
        Carve c{base};
        carve(c, cnt, sample_cols(n, kFlatSampleStride), nominate_sel_k(k), kFlatCap);
        c.take(qbf, cnt * img.dim_pad);
        c.take(counts_wide, cnt * kCountLine);
        rows_c = img.from_codes && n > kFlatCap ? sample_rows(n, kFlatSampleStride) : 0;
        c.take(srows, rows_c * img.dim_pad);
        c.take(snorms, rows_c);
        bytes = c.off;
    }
};
size_t flat_nominate_bf16_scratch(int64_t cnt, int64_t n, const NomImage &img, int k) { return NominateScratch(nullptr, cnt, n, img, k).bytes; }

int32_t flat_nominate_bf16(vg_index *idx, const NomImage &img, bool dot, const float *queries, int64_t cnt, const uint8_t *mask,
                           int64_t mask_stride, int k, char *scratch, hipStream_t st, ProbeNominated *nom)
{
    const NominateScratch s(scratch, cnt, idx->n, img, k);
    NomCall nc{st, dot, {}, cnt, mask, mask_stride};
    // (from the codes the GEMM's "rows" are the codebook; n, the row length and the norms are the decoded rows')
    VG_TRY(gemm_operands(queries, cnt, idx->dim, idx->n, img.norms, img.rows, img.dim_pad, s.qbf, st, &nc.ops, img.scale));
    *nom = s.nom;
    NomCall sc = nc;  // the sample's operands: the image's, or the sampled tiles decoded here
    if (s.rows_c && img.scale) {
        const int groups_pad = img.dim_pad / 16;
        VG_LAUNCH(sq8_sample_rows_kernel, dim3(static_cast<unsigned>((s.rows_c * groups_pad + 255) / 256)), dim3(256), 0, st,
                  reinterpret_cast<const uint4 *>(idx->d_sq_tiles), idx->sq_groups, groups_pad, img.norms, s.rows_c, kFlatSampleStride,
                  reinterpret_cast<uint4 *>(s.srows), s.snorms);
        sc.ops.b = reinterpret_cast<const float *>(s.srows), sc.ops.n = s.rows_c, sc.ops.norms = s.snorms;
    } else if (s.rows_c) {
        const int granules = img.dim_pad / 8;
        VG_LAUNCH(pq_sample_rows_kernel, dim3(static_cast<unsigned>((s.rows_c * granules + 255) / 256)), dim3(256), 0, st, idx->d_pq_rows, idx->n,
                  idx->pq->m, reinterpret_cast<const uint4 *>(img.rows), granules, img.norms, s.rows_c, kFlatSampleStride,
                  reinterpret_cast<uint4 *>(s.srows), s.snorms);
        sc.ops.b = reinterpret_cast<const float *>(s.srows), sc.ops.n = s.rows_c, sc.ops.norms = s.snorms;
    }
    VG_TRY(sample_thresholds(sc, s, s.rows_c ? 1 : kFlatSampleStride, nom->sel_k, nom->thr, idx->n > kFlatCap));
    VG_LAUNCH(flat_thr_cap_kernel, dim3(nc.ucnt()), dim3(64), 0, st, nom->thr, nom->sel_k, queries, idx->dim, img.norm_max);
    VG_HIP(hipMemsetAsync(nom->counts, 0, sizeof(int) * static_cast<size_t>(cnt), st));
    {
        ProfScope prof(idx->ctx, img.scale ? "sq8_codes_gemm" : img.from_codes ? "pq_codes_gemm" : "sq8_nominate_gemm", st);
        GemmArgs a = GemmArgs::append(nc, nom->thr, nom->sel_k, nom->counts, nom->cand, nom->cap).wide(s.counts_wide, idx->ctx->compute_units);
        if (img.scale)
            a.from_sq8_codes(idx->d_sq_tiles, idx->sq_groups);
        else if (img.from_codes)
            a.from_codes(idx->d_pq_rows, idx->pq->m);
        VG_TRY(launch_gemm<2>(a));
    }
    return k <= kNomPickMaxK ? launch_flat_pick(*nom, cnt, nullptr, st) : VG_OK;
}

// ---- the nomination of the threshold search -----------------------------------------------------------------------------------
// The nomination of vg_search_flat_threshold (k_flat_threshold.hip) for batches: the caller's threshold folded into the fused GEMM.
// Per query the append threshold (GEMM score form) is the user's — L2: t - |q|^2, Dot: -t — widened by the verify kernels' error
// bound, or the sample threshold where that is lower; untight[q] = 1 where the user's stands (every row within it is appended
// unless the list overflows), 0 where the sample tightened it, -1 where no bound holds (non-finite rows or query: the proof fails).
// Outputs (ThrNominated, in the scratch): gthr / qnorm / untight [cnt], counts [cnt], cand [cnt * cap] (GEMM keys).
__global__ __launch_bounds__(64) void flat_thr_combine_kernel(const float *__restrict__ uthr, const float *__restrict__ sthr, int sel_k,
                                                              const float *__restrict__ queries, int dim, const float *__restrict__ norm_max,
                                                              float eps_extra, bool dot, float *__restrict__ gthr, float *__restrict__ qnorm,
                                                              int *__restrict__ untight)
{
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    float qn = 0.0f;  // (any order: only feeds the bounds)
    for (int j = lane; j < dim; j += 64) qn = __builtin_fmaf(queries[q * dim + j], queries[q * dim + j], qn);
    for (int off = 32; off > 0; off >>= 1) qn += __shfl_xor(qn, off);
    if (lane != 0) return;
    qnorm[q] = qn;
    const float xmax = norm_max[0];
    const float bound = 2.002f * (qn + xmax);  // above every row's GEMM score (flat_thr_cap_kernel)
    if (!(bound < 1e30f)) {
        gthr[q] = -3.0e38f;  // append nothing; the scan answers the query
        untight[q] = -1;
        return;
    }
    const float t = uthr[q];
    const float eps = (4.0f * (static_cast<float>(dim) * 5.9604645e-8f) + eps_extra) * (qn + xmax) + 1e-30f;
    float ut = (dot ? -t : t - qn) + eps;
    if (!(ut > -bound)) ut = -bound;  // keeps nothing (NaN, or below every score): no row is appended, none is wanted
    if (ut > bound) ut = bound;       // keeps everything: every row is appended (the bf16 tiles need a finite threshold)
    const float st = sthr ? sthr[q * sel_k + sel_k - 1] : INFINITY;
    const bool user = ut <= st;
    gthr[q] = user ? ut : st;
    untight[q] = user ? 1 : 0;
}
// what the nomination keeps to itself: one piece of the caller's arena, for plan.qc queries
struct ThrNomScratch : NomScratch {  // (nom.thr: the sample's thresholds)
    ThrNominated out;
    uint16_t *qbf;
    int *counts_wide;
    ThrNomScratch(char *base, const vg_index *idx, const ThrNomPlan &p, int64_t cnt)
    {
        Carve c{base};
        carve(c, cnt, sample_cols(idx->n, p.sample_stride), p.sel_k, p.cap);
        out.counts = nom.counts, out.cand = nom.cand;
        c.take(out.gthr, cnt);
        c.take(out.qnorm, cnt);
        c.take(out.untight, cnt);
        c.take(qbf, p.bf16 ? cnt * idx->vectors_bf16_dim : 0);
        c.take(counts_wide, p.bf16 ? cnt * kCountLine : 0);
        bytes = c.off;
    }
};
size_t flat_thr_nominate_scratch(const vg_index *idx, const ThrNomPlan &p, int64_t qc) { return ThrNomScratch(nullptr, idx, p, qc).bytes; }

int32_t flat_thr_nominate(vg_index *idx, const ThrNomPlan &p, const float *qp, const float *uthr, int64_t cnt, const uint8_t *m0,
                          int64_t mask_stride, char *scratch, ThrNominated *nominated, hipStream_t st)
{
    const ThrNomScratch s(scratch, idx, p, cnt);
    const ThrNominated &out = *nominated = s.out;
    const bool dot = idx->metric != VG_METRIC_L2;
    NomCall nc{st, dot, fp32_operands(idx, qp), cnt, m0, mask_stride};
    if (p.bf16) VG_TRY(gemm_operands(qp, cnt, idx->dim, idx->n, idx->d_norms, idx->d_vectors_bf16, idx->vectors_bf16_dim, s.qbf, st, &nc.ops));
    const bool use_sample = idx->n > p.cap;  // n <= cap: the list holds every row, the user's threshold stands
    if (use_sample) VG_TRY(sample_thresholds(nc, s, p.sample_stride, p.sel_k, s.nom.thr, true));
    VG_LAUNCH(flat_thr_combine_kernel, dim3(nc.ucnt()), dim3(64), 0, st, uthr, use_sample ? s.nom.thr : nullptr, p.sel_k, qp, idx->dim, idx->d_norm_max,
              p.eps_extra, dot, out.gthr, out.qnorm, out.untight);
    VG_HIP(hipMemsetAsync(out.counts, 0, sizeof(int) * static_cast<size_t>(cnt), st));
    ProfScope prof(idx->ctx, "flat_thr_gemm", st);
    return launch_gemm<2>(GemmArgs::append(nc, out.gthr, 1, out.counts, out.cand, p.cap).wide(p.bf16 ? s.counts_wide : nullptr, idx->ctx->compute_units));
}

// the work list of the queries whose proof failed (todo[0] = how many, todo[1 ..] = which) and the statistics
// (counts, or null: the chunk's candidate counts, for vg_index_flat_appended)
int32_t launch_flat_todo(const int *flags, const int *always, int cnt, int *todo, unsigned long long *stats, hipStream_t st, const int *counts)
{
    VG_LAUNCH(flat_todo_kernel, dim3(1), dim3(256), 0, st, flags, always, cnt, todo, stats, counts);
    return VG_OK;
}
}  // namespace vg

VG_API int32_t vg_search_flat(vg_index *idx, const float *queries, int64_t nq, int32_t k, uint32_t *ids,
                              float *scores, void *stream)
{
    return vg::flat_search_masked(idx, queries, nq, k, nullptr, 0, ids, scores, stream);
}

namespace vg {
int32_t append_bf16_rows(vg_index *idx, int64_t from, int64_t to, hipStream_t st)
{
    const int64_t count = (to - from) * idx->vectors_bf16_dim;
    if (count <= 0) return VG_OK;
    VG_LAUNCH(f32_to_bf16_pad_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, st,
              idx->d_vectors + from * idx->dim, to - from, idx->dim, idx->vectors_bf16_dim,
              idx->d_vectors_bf16 + from * idx->vectors_bf16_dim);
    return VG_OK;
}
}  // namespace vg

VG_API int32_t vg_index_flat_appended(vg_index *idx, int64_t *appended, void *stream)
{
    VG_CHECK(idx && appended, VG_ERR_INVALID_ARG, "vg_index_flat_appended: NULL index or pointer");
    VG_CHECK(idx->d_flat_stats, VG_ERR_INVALID_ARG, "vg_index_flat_appended: no fp32 vectors attached");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    unsigned long long h = 0;
    VG_HIP(hipMemcpyAsync(&h, idx->d_flat_stats + 3, sizeof h, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    *appended = static_cast<int64_t>(h);
    return VG_OK;
}

VG_API int32_t vg_index_enable_bf16_filter(vg_index *idx, int32_t on, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_enable_bf16_filter: NULL index");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    if (idx->d_vectors_bf16) {
        VG_HIP(hipStreamSynchronize(st));
        VG_HIP(hipFree(idx->d_vectors_bf16));
        idx->d_vectors_bf16 = nullptr;
    }
    idx->bf16_cap = 0;
    if (!on) return VG_OK;
    VG_CHECK(idx->d_vectors, VG_ERR_NOT_READY, "vg_index_enable_bf16_filter: index has no fp32 vectors");
    // rows of whole K steps (2 * kGemmBK = 64 bfloat16): the dimensions from dim on are zeros, which add nothing to a dot product
    idx->vectors_bf16_dim = (idx->dim + 2 * vg::kGemmBK - 1) / (2 * vg::kGemmBK) * (2 * vg::kGemmBK);
    const int64_t count = idx->n * idx->vectors_bf16_dim;
    VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_vectors_bf16), static_cast<size_t>(count) * sizeof(uint16_t)));
    VG_LAUNCH(vg::f32_to_bf16_pad_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, st, idx->d_vectors,
              idx->n, idx->dim, idx->vectors_bf16_dim, idx->d_vectors_bf16);
    VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}

VG_API int32_t vg_index_flat_stats(vg_index *idx, int64_t *queries, int64_t *exhaustive, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_flat_stats: NULL index");
    VG_CHECK(idx->d_flat_stats, VG_ERR_INVALID_ARG, "vg_index_flat_stats: no fp32 vectors attached");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    unsigned long long h[2] = {0, 0};
    VG_HIP(hipMemcpyAsync(h, idx->d_flat_stats, sizeof h, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    if (queries) *queries = static_cast<int64_t>(h[0]);
    if (exhaustive) *exhaustive = static_cast<int64_t>(h[1]);
    return VG_OK;
}

VG_API int32_t vg_index_flat_retried(vg_index *idx, int64_t *retried, void *stream)
{
    VG_CHECK(idx && retried, VG_ERR_INVALID_ARG, "vg_index_flat_retried: NULL index or pointer");
    VG_CHECK(idx->d_flat_stats, VG_ERR_INVALID_ARG, "vg_index_flat_retried: no fp32 vectors attached");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    unsigned long long h = 0;
    VG_HIP(hipMemcpyAsync(&h, idx->d_flat_stats + 2, sizeof h, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    *retried = static_cast<int64_t>(h);
    return VG_OK;
}
