// vg_nominate.hpp — the batched search through a bfloat16 nomination image, shared by the quantizers that have one
// (vg_index_enable_sq8_nomination and _from_codes, k_sq8_scan.hip; vg_index_enable_pq_nomination and _from_codes, k_pq_nominate.hip).
// The image holds a quantizer's DECODED rows x^ rounded to bfloat16 with their norms (NomImage, vg_internal.hpp); the fused flat
// search's nomination runs on it (k_flat.hip flat_nominate_bf16: threshold from a row sample, bf16 MFMA GEMM, the 64 best per
// query), the verify kernels below re-score the nominees with the reference's own arithmetic on the CODES (the quantizer's Row)
// and prove that no row outside them can enter the k best: outside rows have GEMM score >= tau, and
// |GEMM score + |q|^2 - offset - exact score| <= Row::eps, offset = the Row's per-query constant between the GEMM's score space and
// the exact one (zero for an image of the decoded rows).  A query whose proof fails is searched again by the caller's exact path.
#pragma once

#include <algorithm>
#include <vector>

#include "vg_device.hpp"
#include "vg_internal.hpp"

namespace vg {

// k <= 48: the 64 best nominees are re-scored (nominated_verify_kernel); up to 256: everything below the threshold
// (nominated_verify_sort_kernel) — the 8th best of the 1/64 row sample passes ~512 rows, the 16th ~1024, the 32nd ~2048.  (The
// proof wants the threshold 2^-7 (|q|^2 + |x^|^2) above the k-th score: ~512 rows for k = 100 left enough queries to the scan —
// random-normal rows, 1M x 768 — that the SQ8 batch took 8.3 ms, ~1024 rows 3 ms.)
constexpr int kNomPickMaxK = 48, kNomMaxK = 256;
inline int nominate_sel_k(int k) { return k <= kNomPickMaxK ? 8 : k <= 128 ? 16 : 32; }

struct GemmGroup;  // vg_flat_gemm.hpp
// k_flat.hip
// cnt queries' nomination for their k best on `img`, *nom and all it points to in `scratch` (flat_nominate_bf16_scratch bytes)
// (img.from_codes, a nomination from the codes: unfiltered; PQ: L2; SQ8, img.scale: L2 and Dot, more than 128 queries)
size_t flat_nominate_bf16_scratch(int64_t cnt, int64_t n, const NomImage &img, int k);
int32_t flat_nominate_bf16(vg_index *idx, const NomImage &img, bool dot, const float *queries, int64_t cnt, const uint8_t *mask,
                           int64_t mask_stride, int k, char *scratch, hipStream_t st, ProbeNominated *nom);
size_t flat_probe_gemm_scratch_bytes(int64_t pairs, int64_t ns_max, int k, int bf16_dim);
int32_t flat_probe_gemm(vg_index *idx, const float *pair_queries, int64_t pairs, const GemmGroup *groups, const int64_t *const first_block[4],
                        int ngroups, const int64_t grid[4], int sample_stride, int64_t ns_max, int k, uint32_t *pair_ids,
                        float *pair_scores, int *fail, char *scratch, const uint8_t *mask, const int64_t *mask_off, hipStream_t st,
                        const NomImage &img, ProbeNominated *nominated);
// k_sq8_scan.hip
int32_t launch_sq8_verify(vg_index *idx, const float *queries, int64_t nq, const ProbeNominated &nom, int k, uint32_t *ids, float *scores,
                          int *fail, hipStream_t st);
bool sq8_nomination_applies(const vg_index *idx, const float *d_queries, int64_t nq, int k, const uint8_t *mask);
int32_t sq8_nominated_pass(vg_index *idx, const float *q, int64_t nq, int k, const uint8_t *mask, int64_t mask_stride, uint32_t *oid,
                           float *osc, hipStream_t st, std::vector<int> &failed);
// k_pq_nominate.hip (ascending table sums over the whole segment: mask null, desc false, or the batch does not apply)
bool pq_nomination_applies(const vg_index *idx, const float *d_queries, int64_t nq, int k, const uint8_t *mask, bool desc);
int32_t pq_nominated_pass(vg_index *idx, const float *q, int64_t nq, int k, uint32_t *oid, float *osc, hipStream_t st, std::vector<int> &failed);

// Builds the nomination state of n rows of dim elements into `img` (empty): its body of body_bytes (NomImage::body_bytes — the
// decoded rows, or from_codes the decoded codebook), the norms and norm_max.  launch(const NomImage &, int *norm_max_bits) launches
// the quantizer's build kernels, which write the body (a row's tail from dim on zeros), the rows' norms and atomicMax their largest
// into norm_max (zeroed here).  The arrays are published together, after all of it is built: a failure half way leaves the index
// as it was (the batch searches test `rows` alone — ADVICE r05: a failed second allocation left it set next to null norms).
inline int nom_dim_pad(int dim) { return (dim + 63) & ~63; }  // whole K steps of the bf16 GEMM; the padding is zeros
template <class Launch>
int32_t nom_build(NomImage &img, int64_t n, int dim, int64_t body_bytes, bool from_codes, hipStream_t st, Launch launch)
{
    NomImage b;
    b.dim_pad = nom_dim_pad(dim);
    b.from_codes = from_codes;
    b.body = body_bytes;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.rows), static_cast<size_t>(body_bytes));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b.norms), static_cast<size_t>(n) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b.norm_max), sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(b.norm_max, 0, sizeof(float), st);
    if (e == hipSuccess) {
        launch(static_cast<const NomImage &>(b), reinterpret_cast<int *>(b.norm_max));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(b.rows);
        (void)hipFree(b.norms);
        (void)hipFree(b.norm_max);
        VG_HIP(e);
    }
    img = b;
    return VG_OK;
}

// per query: the exact score of its 64 nominated rows (Row::score), the k best by (score, row id), and the proof.
// Row: dim (the queries' row length), score(q, qv, id) — row id's exact score for query q (qv: its values) —,
// eps(qn, norm_max) — |s~ + |q|^2 - offset - exact score| for any row, the margin of the proof — and kShifted: whether the GEMM's
// score space has a per-query constant c, L2 exact ~ s~ + |q|^2 - 2 c, Dot (the scores are -q.x) exact ~ s~ - c; then shift(qv,
// lane) is the lane's share of c, summed over the wave.  The images of the decoded rows have none (their kernels are what they
// were); the SQ8 nomination from the codes multiplies centred codes and has c = q.mid (Sq8CodesRow, k_sq8_scan.hip).  A NaN c
// fails the proof.
// the Row's score-space constant (see nominated_verify_kernel): its lanes' shares summed over the wave; Row::kShifted false: none
template <class Row>
__device__ __forceinline__ float wave_shift(const Row &row, const float *qv, int lane)
{
    if constexpr (Row::kShifted) {
        float c = row.shift(qv, lane);
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
        return c;
    } else {
        return 0.0f;
    }
}
// what the k-th exact score is compared with: tau in the exact score's space
template <class Row, bool DOT>
__device__ __forceinline__ float shifted_tau(float tau, float qn, float shift)
{
    const float t = DOT ? -tau : tau + qn;
    if constexpr (Row::kShifted)
        return DOT ? t + shift : t - 2.0f * shift;
    else
        return t;
}

template <class Row, bool DOT>
__global__ __launch_bounds__(64) void nominated_verify_kernel(Row row, const float *__restrict__ queries, const float *__restrict__ norm_max,
                                                              const uint32_t *__restrict__ cand_ids, const float *__restrict__ cand_scores, int k,
                                                              uint32_t *__restrict__ ids, float *__restrict__ scores, int *__restrict__ fail,
                                                              const float *__restrict__ thr, const int *__restrict__ counts, int cap,
                                                              int thr_stride)
{
    constexpr int kc = 64;
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const int dim = row.dim;
    const float *qv = queries + q * dim;
    const uint32_t id = cand_ids[q * kc + lane];
    uint64_t key = kKeyMax;
    if (id != VG_INVALID_ID) key = make_key(row.score(q, qv, id), id, DOT);
    WaveTopK tk;
    tk.init(k);
    tk.offer(key, lane);
    float qn = 0.0f;
    for (int j = lane; j < dim; j += 64) qn = __builtin_fmaf(qv[j], qv[j], qn);
    for (int off = 32; off > 0; off >>= 1) qn += __shfl_xor(qn, off);
    const float shift = wave_shift(row, qv, lane);
    const uint64_t kth = readlane_u64(tk.list, k - 1);
    const float tq = thr[q * thr_stride + (thr_stride - 1)];
    const int cnt = counts[q];
    bool ok = cnt <= cap && shift == shift;  // overflow: rows below the threshold were dropped
    const float tau = cnt > kc ? fminf(tq, cand_scores[q * kc + (kc - 1)]) : tq;
    const bool have_all = tq == INFINITY && cnt <= kc;
    if (ok && !have_all && tau != INFINITY) {
        const float eps = row.eps(qn, norm_max[0]);
        if (kth == kKeyMax)
            ok = false;
        else if (DOT)
            ok = key_score(kth, true) > shifted_tau<Row, true>(tau, qn, shift) + eps;  // outside rows: -q.x >= tau
        else
            ok = key_score(kth, false) < shifted_tau<Row, false>(tau, qn, shift) - eps;
    }
    if (lane < k) {
        const uint64_t e = tk.list;
        ids[q * k + lane] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        scores[q * k + lane] = e == kKeyMax ? (DOT ? -INFINITY : INFINITY) : key_score(e, DOT);
    }
    if (lane == 0) fail[q] = ok ? 0 : 1;
}

// The same for k beyond the 64-candidate budget (flat_verify_sort_kernel's counterpart): EVERY appended row is re-scored — one
// lane per row — and sorted; what is left to argue about is what the threshold excluded, so the proof compares the k-th exact
// score with the threshold itself.  Dynamic LDS: cap keys.
template <class Row, bool DOT>
__global__ __launch_bounds__(256) void nominated_verify_sort_kernel(Row row, const float *__restrict__ queries, const float *__restrict__ norm_max,
                                                                    const uint64_t *__restrict__ cand, const int *__restrict__ counts, int cap, int k,
                                                                    uint32_t *__restrict__ ids, float *__restrict__ scores, int *__restrict__ fail,
                                                                    const float *__restrict__ thr, int thr_stride)
{
    extern __shared__ uint64_t sortbuf[];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int dim = row.dim;
    const float *qv = queries + q * dim;
    const int total = counts[q];
    const int cnt = total < cap ? total : cap;
    int n2 = 64;
    while (n2 < cnt) n2 <<= 1;
    for (int c = tid; c < cnt; c += 256) {
        const uint32_t id = key_row(cand[q * cap + c]);
        sortbuf[c] = make_key(row.score(q, qv, id), id, DOT);
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
    const float shift = wave_shift(row, qv, lane);
    const uint64_t kth = k - 1 < n2 ? sortbuf[k - 1] : kKeyMax;
    const float tau = thr[q * thr_stride + (thr_stride - 1)];
    bool ok = total <= cap && shift == shift;
    if (ok && tau != INFINITY) {  // (tau == +Inf: no threshold was set, every accepted row was appended)
        const float eps = row.eps(qn, norm_max[0]);
        if (kth == kKeyMax)
            ok = false;
        else if (DOT)
            ok = key_score(kth, true) > shifted_tau<Row, true>(tau, qn, shift) + eps;
        else
            ok = key_score(kth, false) < shifted_tau<Row, false>(tau, qn, shift) - eps;
    }
    if (lane == 0) fail[q] = ok ? 0 : 1;
}

// the verify pair over nq queries' nominations (nom; norm_max: the image's)
template <bool DOT, class Row>
int32_t launch_nominated_verify(const Row &row, const float *queries, const float *norm_max, int64_t nq, const ProbeNominated &nom, int k,
                                uint32_t *ids, float *scores, int *fail, hipStream_t st)
{
    if (k > kNomPickMaxK) {
        auto kern = nominated_verify_sort_kernel<Row, DOT>;
        VG_LAUNCH(kern, dim3(static_cast<unsigned>(nq)), dim3(256), sizeof(uint64_t) * static_cast<size_t>(nom.cap), st, row, queries,
                  norm_max, nom.cand, nom.counts, nom.cap, k, ids, scores, fail, nom.thr, nom.sel_k);
        return VG_OK;
    }
    auto kern = nominated_verify_kernel<Row, DOT>;
    VG_LAUNCH(kern, dim3(static_cast<unsigned>(nq)), dim3(64), 0, st, row, queries, norm_max, nom.cand_id, nom.cand_sc, k, ids, scores, fail,
              nom.thr, nom.counts, nom.cap, nom.sel_k);
    return VG_OK;
}

// the queries (offset by `base`) whose device fail flag d_fail[0, cnt) is set, appended to `failed` (waits for the stream)
inline int32_t failed_list(const int *d_fail, int64_t cnt, int64_t base, hipStream_t st, std::vector<int> &failed)
{
    std::vector<int> h(static_cast<size_t>(cnt));
    VG_HIP(hipMemcpyAsync(h.data(), d_fail, sizeof(int) * static_cast<size_t>(cnt), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < cnt; i++)
        if (h[static_cast<size_t>(i)]) failed.push_back(static_cast<int>(base + i));
    return VG_OK;
}

// The nomination + exact re-score + proof for a batch (device buffers; dot: the scores are -q.x; mask: a device row filter per
// query / for the batch, or null): writes every query's k results and lists the queries whose proof failed — the caller searches
// those again (rescan_failed).  4096 queries a pass.  verify(queries, cnt, nom, extra, ids, scores, fail) re-scores and proves a
// pass's nominations; extra: extra_floats per query of the pass's scratch (the PQ distance tables).
template <class Verify>
int32_t nominated_pass(vg_index *idx, const NomImage &img, bool dot, const float *q, int64_t nq, int k, const uint8_t *mask,
                       int64_t mask_stride, size_t extra_floats, uint32_t *oid, float *osc, hipStream_t st, std::vector<int> &failed,
                       Verify verify)
{
    for (int64_t q0 = 0; q0 < nq; q0 += 4096) {
        const int64_t cnt = std::min<int64_t>(4096, nq - q0);
        ArenaCall ar(idx->ctx, st);
        const int i_scr = ar.add(flat_nominate_bf16_scratch(cnt, idx->n, img, k));
        const int i_fail = ar.add(sizeof(int) * static_cast<size_t>(cnt));
        const int i_extra = ar.add(sizeof(float) * static_cast<size_t>(cnt) * extra_floats);
        VG_TRY(ar.commit());
        int *fail = ar.get<int>(i_fail);
        const float *qq = q + q0 * idx->dim;
        ProbeNominated nom;
        VG_TRY(flat_nominate_bf16(idx, img, dot, qq, cnt, mask ? mask + q0 * mask_stride : nullptr, mask_stride, k, ar.get<char>(i_scr), st, &nom));
        VG_TRY(verify(qq, cnt, nom, ar.get<float>(i_extra), oid + q0 * k, osc + q0 * k, fail));
        VG_TRY(failed_list(fail, cnt, q0, st, failed));
    }
    return VG_OK;
}

// The failed queries of a batch searched again: their queries (and, with a filter per query, their filters of mask_bytes) gathered,
// search(queries, nf, mask, mask_stride, ids, scores) run on them — the caller's exact path — and their k results scattered back
// into oid / osc.  mask: the batch's device filter (per query at mask_stride, or one for all with stride 0), or null.
template <class Search>
int32_t rescan_failed(const std::vector<int> &failed, const float *q, int dim, int k, const uint8_t *mask, int64_t mask_stride,
                      int64_t mask_bytes, uint32_t *oid, float *osc, hipStream_t st, Search search)
{
    if (failed.empty()) return VG_OK;
    const int64_t nf = static_cast<int64_t>(failed.size());
    const bool per_query = mask && mask_stride;
    DevTmp<float> fq;
    DevTmp<uint32_t> fid;
    DevTmp<float> fsc;
    DevTmp<uint8_t> fm;
    VG_TRY(fq.init(static_cast<size_t>(nf) * dim, st));
    VG_TRY(fid.init(static_cast<size_t>(nf) * k, st));
    VG_TRY(fsc.init(static_cast<size_t>(nf) * k, st));
    VG_TRY(fm.init(per_query ? static_cast<size_t>(nf) * mask_bytes : 0, st));
    for (int64_t i = 0; i < nf; i++) {
        const int64_t src = failed[static_cast<size_t>(i)];
        VG_HIP(hipMemcpyAsync(fq.ptr + i * dim, q + src * dim, sizeof(float) * dim, hipMemcpyDeviceToDevice, st));
        if (per_query)
            VG_HIP(hipMemcpyAsync(fm.ptr + i * mask_bytes, mask + src * mask_stride, static_cast<size_t>(mask_bytes), hipMemcpyDeviceToDevice,
                                  st));
    }
    VG_TRY(search(fq.ptr, nf, per_query ? fm.ptr : mask, mask_stride ? mask_bytes : int64_t(0), fid.ptr, fsc.ptr));
    for (int64_t i = 0; i < nf; i++) {
        const int64_t at = static_cast<int64_t>(failed[static_cast<size_t>(i)]) * k;
        VG_HIP(hipMemcpyAsync(oid + at, fid.ptr + i * k, sizeof(uint32_t) * k, hipMemcpyDeviceToDevice, st));
        VG_HIP(hipMemcpyAsync(osc + at, fsc.ptr + i * k, sizeof(float) * k, hipMemcpyDeviceToDevice, st));
    }
    return VG_OK;
}

}  // namespace vg
