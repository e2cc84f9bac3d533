// k_rabitq_nominate.hip — vg_search_rabitq batches through an int8 matrix-core nomination (vg_index_enable_rabitq_nomination).
//
// A Hamming distance is a dot product of +-1 vectors: with the sign bits of a query and a row expanded to int8 (bit set: +1, clear:
// -1), s = sum s_q s_y = K - 2 h over the K = rq_groups * 128 bit positions of the index's code tiles (zero pad bits are -1 on both
// sides and agree, as they do under the scan's xor), and v_mfma_i32_32x32x32_i8 accumulates it EXACTLY.  So, unlike the bfloat16
// nominations (vg_nominate.hpp), the product carries no rounded operand and no margin: what is left to prove is that the list of
// rows at or below a threshold is complete.  Per pass of up to 4096 queries (rabitq_nominated_pass):
//   1. threshold: the rows of every 64th 64-row tile scored exactly (rabitq_scan_mq_kernel over the sampled tiles, k_rabitq.hip);
//      tau_q = the nominate_sel_k(k)-th best of them, +Inf when the sample has fewer or the index has no more than 64 tiles
//   2. the queries' sign bits expanded once into the GEMM's LDS image (rabitq_nom_prep_kernel)
//   3. GEMM (rabitq_nom_gemm_kernel): persistent 256-query x 256-row tiles, a K step = 128 bits = one 16-byte group of the code
//      tiles per row, expanded in registers; the epilogue appends (row, h) to the query's list when the SCREEN (vg_rabitq.hpp)
//      says the exact score may be <= tau_q — a handful of packed fp32 operations per pair instead of the formula's division
//   4. verify (rabitq_nom_verify_kernel): every listed row re-scored from the codes with popcount + rq_formula, the k best by
//      (score, row id), and the proof: the list did not overflow (kRnCap keys), and at least k listed rows have exact score <=
//      tau_q — or tau_q = +Inf, when every row was listed.  Every unlisted row then has exact score > tau_q >= the k-th.  No eps.
//   5. the queries whose proof failed go through the scan (vg_search_rabitq, k_rabitq.hip) and are counted (`rescanned`).
// Nothing is resident beyond the code tiles and norms the index holds (held_bytes = 0).  Enabling looks at the stored norms once: a
// NEGATIVE one (the caller's bytes) breaks the screen's inequality, and such an index keeps the scan for every batch.  A row
// permutation (vg_vamana_reorder_bfs) changes neither, so the mode stays correct across it.
#include <algorithm>
#include <vector>

#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_nominate.hpp"
#include "vg_rabitq.hpp"
#include "vg_search.hpp"

namespace vg {

constexpr int kRnTile = 256;                          // queries and rows of a tile
constexpr int kRnThreads = 512;                       // 8 waves: 2 (128 queries each) x 4 (64 rows each)
constexpr int kRnStep = 128;                          // bytes (= int8 elements) of a row or query per K step
constexpr int kRnImage = kRnTile * kRnStep;           // one operand's LDS image of a step: 32 KiB
constexpr int kRnLds = 4 * kRnImage + 2 * kRnTile * static_cast<int>(sizeof(float));  // two steps of both images + the rows' norms, twice
constexpr int kRnCap = 4096;                          // keys kept per query (the siblings' capacity)
constexpr int kRnCountStride = 32;                    // a query's counter every 128 bytes
// Batches from this many (query, row) pairs up take the nomination (test hook VG_RABITQ_NOM_ALWAYS: any number).
// tools/rabitq_nominate_time.py; DESIGN.md "RaBitQ batch nomination".
constexpr int64_t kRabitqNomMinPairs = 12000000;

typedef int rn_i4 __attribute__((ext_vector_type(4)));
typedef int rn_i16 __attribute__((ext_vector_type(16)));
typedef float rn_f2 __attribute__((ext_vector_type(2)));

// byte offset of 16-byte chunk ch (0..7) of row r in a [256][128 B] image: the XOR spreads 16 consecutive rows' reads of one chunk
// over the 16 slots of the 256-byte bank row (rows r, r + 1 are its halves)
__device__ __forceinline__ int rn_off(int r, int ch) { return r * kRnStep + ((ch ^ ((r >> 1) & 7)) << 4); }

// The queries' LDS image [step][qpad][128 B] (chunks at rn_off's places, so that the GEMM's fill is a linear copy), their norms and
// thresholds.  Queries from cnt to qpad: no bits, NaN threshold (nothing compares <= NaN).  One thread per (query, step, chunk).
__global__ __launch_bounds__(256) void rabitq_nom_prep_kernel(const uint8_t *__restrict__ qcodes, int nb, int groups, int cnt, int qpad,
                                                              const float *__restrict__ thr, int sel_k, uint8_t *__restrict__ qimg,
                                                              float *__restrict__ qn, float *__restrict__ tau)
{
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (gid >= static_cast<int64_t>(qpad) * groups * 8) return;
    const int ch = static_cast<int>(gid & 7);
    const int q = static_cast<int>((gid >> 3) % qpad);
    const int s = static_cast<int>((gid >> 3) / qpad);
    uint32_t bits = 0;
    if (q < cnt) {
        const uint8_t *qc = qcodes + static_cast<int64_t>(q) * (nb + 4);
        const int at = s * 16 + ch * 2;
        if (at < nb) bits = qc[at] | (static_cast<uint32_t>(qc[at + 1]) << 8);  // (nb is even)
    }
    *reinterpret_cast<uint4 *>(qimg + (static_cast<int64_t>(s) * qpad + (q & ~255)) * kRnStep + rn_off(q & 255, ch)) = rn_expand16(bits);
    if (s == 0 && ch == 0) {
        qn[q] = q < cnt ? rq_code_norm(qcodes + static_cast<int64_t>(q) * (nb + 4), nb) : 0.0f;
        tau[q] = q < cnt ? (thr ? thr[static_cast<int64_t>(q) * sel_k + (sel_k - 1)] : INFINITY) : __uint_as_float(0x7FC00000u);
    }
}

// The GEMM.  Workgroup b takes tiles b, b + gridDim.x, ... of the (row tile, query tile) grid, query tiles innermost (neighbouring
// workgroups share a row tile).  Per K step s the 256 queries' and 256 rows' 128 int8 lie in LDS (two buffers: step s + 1 is loaded
// into registers before step s is multiplied and written behind it, one barrier per step); wave (wq, wr) multiplies rows wr * 64 ..
// + 63 (A operand) by queries wq * 128 .. + 127 (B operand): 2 x 4 blocks of 32 x 32, four v_mfma_i32_32x32x32_i8 per block and step.
// Both operands take the same 16-byte chunk of the step per lane half, so the sum runs over all 128 positions whatever order the
// instruction gives them (tools/ubench/mfma_i8_probe.hip checks the maps with asymmetric integer data all the same).  Result
// register r of lane l: query l & 31, row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the block.
__global__ __launch_bounds__(kRnThreads) void rabitq_nom_gemm_kernel(const uint8_t *__restrict__ tiles, const float *__restrict__ norms, int64_t n,
                                                                     int64_t n_tiles, int groups, const uint8_t *__restrict__ qimg, int qpad,
                                                                     const float *__restrict__ qn, const float *__restrict__ tau, float invd,
                                                                     int *__restrict__ counts, uint64_t *__restrict__ cand)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rn_smem[];
    float *yn_lds = reinterpret_cast<float *>(rn_smem + 4 * kRnImage);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave & 1, wr = wave >> 1;
    const int n_qt = qpad / kRnTile;
    const int64_t total = ((n + kRnTile - 1) / kRnTile) * n_qt;
    const int fr = tid & 255, fhalf = tid >> 8;  // the fill: thread (fr, fhalf) expands half of row fr's 16 bytes
    const float k_half = static_cast<float>(groups * 64);
    int parity = 0;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x, parity ^= 1) {
        const int q0 = static_cast<int>(t % n_qt) * kRnTile;
        const int64_t rt = t / n_qt, row0 = rt * kRnTile;
        float *yn = yn_lds + parity * kRnTile;
        if (tid < kRnTile) yn[tid] = row0 + tid < n ? norms[row0 + tid] : __uint_as_float(0x7FC00000u);  // past the end: NaN, never listed
        uint4 qreg0, qreg1, qreg2, qreg3;
        uint2 rreg;
        const int64_t ftile = rt * 4 + (fr >> 6);
        auto load = [&](int s) {
            const uint4 *src = reinterpret_cast<const uint4 *>(qimg + (static_cast<int64_t>(s) * qpad + q0) * kRnStep);
            qreg0 = src[tid];
            qreg1 = src[kRnThreads + tid];
            qreg2 = src[2 * kRnThreads + tid];
            qreg3 = src[3 * kRnThreads + tid];
            rreg = make_uint2(0u, 0u);
            if (ftile < n_tiles) rreg = *reinterpret_cast<const uint2 *>(tiles + ((ftile * groups + s) * 64 + (fr & 63)) * 16 + fhalf * 8);
        };
        auto store = [&](int buf) {
            unsigned char *qb = rn_smem + buf * 2 * kRnImage, *rb = qb + kRnImage;
            reinterpret_cast<uint4 *>(qb)[tid] = qreg0;
            reinterpret_cast<uint4 *>(qb)[kRnThreads + tid] = qreg1;
            reinterpret_cast<uint4 *>(qb)[2 * kRnThreads + tid] = qreg2;
            reinterpret_cast<uint4 *>(qb)[3 * kRnThreads + tid] = qreg3;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t w = j < 2 ? rreg.x : rreg.y;
                *reinterpret_cast<uint4 *>(rb + rn_off(fr, fhalf * 4 + j)) = rn_expand16((w >> (16 * (j & 1))) & 0xFFFFu);
            }
        };
        rn_i16 acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 4; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[a][b][r] = 0;
        load(0);
        store(0);
        __syncthreads();
        for (int s = 0; s < groups; s++) {
            const bool more = s + 1 < groups;
            if (more) load(s + 1);
            const unsigned char *qb = rn_smem + (s & 1) * 2 * kRnImage, *rb = qb + kRnImage;
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const int ch = 2 * kk + (lane >> 5);
                rn_i4 a[2], b[4];
#pragma unroll
                for (int i = 0; i < 2; i++) a[i] = *reinterpret_cast<const rn_i4 *>(rb + rn_off(wr * 64 + i * 32 + (lane & 31), ch));
#pragma unroll
                for (int i = 0; i < 4; i++) b[i] = *reinterpret_cast<const rn_i4 *>(qb + rn_off(wq * 128 + i * 32 + (lane & 31), ch));
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
            }
            if (more) store((s + 1) & 1);
            __syncthreads();
        }
        // the screen (vg_rabitq.hpp), two rows at a time in packed fp32
        const rn_f2 invd2 = {invd, invd}, khalf2 = {k_half, k_half}, mhalf2 = {-0.5f, -0.5f};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int q = q0 + wq * 128 + j * 32 + (lane & 31);
            const float qnv = qn[q], tq = tau[q];
            const float a4 = 4.0f * qnv;
            const rn_f2 qn2 = {qnv, qnv}, a2 = {a4, a4};
#pragma unroll
            for (int i = 0; i < 2; i++) {
#pragma unroll
                for (int r4 = 0; r4 < 4; r4++) {
                    const int rl = wr * 64 + i * 32 + 8 * r4 + 4 * (lane >> 5);
                    const float4 y = *reinterpret_cast<const float4 *>(yn + rl);
#pragma unroll
                    for (int p = 0; p < 2; p++) {
                        const rn_f2 y2 = p ? rn_f2{y.z, y.w} : rn_f2{y.x, y.y};
                        const int s0 = acc[i][j][4 * r4 + 2 * p], s1 = acc[i][j][4 * r4 + 2 * p + 1];
                        const rn_f2 sf = {static_cast<float>(s0), static_cast<float>(s1)};
                        const rn_f2 hf = __builtin_elementwise_fma(sf, mhalf2, khalf2);  // h = (K - s) / 2, exact
                        const rn_f2 t1 = qn2 - y2;
                        const rn_f2 t1sq = t1 * t1;
                        rn_f2 c = a2 * y2;
                        c = c * invd2;
                        const rn_f2 sc = t1sq + c * hf;
                        if (sc.x <= tq || sc.y <= tq) {
#pragma unroll
                            for (int e = 0; e < 2; e++) {
                                if ((e ? sc.y : sc.x) <= tq) {
                                    const uint32_t h = static_cast<uint32_t>((groups * 128 - (e ? s1 : s0)) >> 1);
                                    const uint32_t row = static_cast<uint32_t>(row0 + rl + 2 * p + e);
                                    const int pos = atomicAdd(counts + static_cast<int64_t>(q) * kRnCountStride, 1);
                                    if (pos < kRnCap) cand[static_cast<int64_t>(q) * kRnCap + pos] = (static_cast<uint64_t>(h) << 32) | row;
                                }
                            }
                        }
                    }
                }
            }
        }
    }
}

// Per query: every listed row re-scored from the row-major codes as the scan scores it, sorted by (score, row id), the k best written,
// and the proof (the head of this file).  check: each key's h against the popcount, disagreements added to *mismatched.
__global__ __launch_bounds__(256) void rabitq_nom_verify_kernel(const uint8_t *__restrict__ rows, const uint8_t *__restrict__ qcodes, int nb, int dim,
                                                                const float *__restrict__ tau, const int *__restrict__ counts,
                                                                const uint64_t *__restrict__ cand, int k, uint32_t *__restrict__ ids,
                                                                float *__restrict__ scores, int *__restrict__ fail, int check,
                                                                int *__restrict__ mismatched)
{
    extern __shared__ uint64_t rn_sort[];
    __shared__ int n_le, n_bad;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const int total = counts[q * kRnCountStride];
    const int cnt = total < kRnCap ? total : kRnCap;
    int n2 = 64;
    while (n2 < cnt) n2 <<= 1;
    if (tid == 0) n_le = n_bad = 0;
    __syncthreads();
    const uint8_t *qc = qcodes + q * (nb + 4);
    const float qnv = rq_code_norm(qc, nb), tq = tau[q], dimf = static_cast<float>(dim);
    int le = 0, bad = 0;
    for (int c = tid; c < cnt; c += 256) {
        const uint64_t key = cand[q * kRnCap + c];
        const uint32_t id = static_cast<uint32_t>(key);
        const uint8_t *rc = rows + static_cast<int64_t>(id) * (nb + 4);
        const int h = hamming_bytes(qc, rc, nb);
        const float sc = rq_formula(qnv, rq_code_norm(rc, nb), dimf, static_cast<float>(h));
        rn_sort[c] = make_key(sc, id, false);
        le += sc <= tq ? 1 : 0;
        bad += static_cast<uint32_t>(h) != static_cast<uint32_t>(key >> 32) ? 1 : 0;
    }
    for (int i = cnt + tid; i < n2; i += 256) rn_sort[i] = kKeyMax;
    if (le) atomicAdd(&n_le, le);
    if (check && bad) atomicAdd(&n_bad, bad);
    __syncthreads();
    bitonic_sort_lds(rn_sort, n2, tid, 256);
    for (int i = tid; i < k; i += 256) {
        const uint64_t e = i < n2 ? rn_sort[i] : kKeyMax;
        ids[q * k + i] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        scores[q * k + i] = e == kKeyMax ? INFINITY : key_score(e, false);
    }
    if (tid == 0) {
        fail[q] = total <= kRnCap && (tq == INFINITY || n_le >= k) ? 0 : 1;
        if (check && n_bad) atomicAdd(mismatched, n_bad);
    }
}

// whether one of n stored norms is negative
__global__ __launch_bounds__(256) void rabitq_nom_negative_kernel(const float *__restrict__ norms, int64_t n, int *__restrict__ flag)
{
    bool neg = false;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) neg = neg || norms[i] < 0.0f;
    if (__ballot(neg) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

bool rabitq_nomination_applies(const vg_index *idx, int64_t nq, int k)
{
    if (!idx->rq_nom_on || idx->rq_nom_negative || nq <= 128 || k > kNomMaxK || idx->n <= k) return false;
    return nq * idx->n >= kRabitqNomMinPairs || hook(kHookRabitqNomAlways);
}

int32_t rabitq_nomination_drop(vg_index *idx)
{
    idx->rq_nom_on = idx->rq_nom_negative = false;
    idx->rq_nom_rescanned = idx->rq_nom_mismatched = 0;
    return VG_OK;
}

int32_t rabitq_nominated_pass(vg_index *idx, const uint8_t *qcodes, int64_t nq, int k, uint32_t *oid, float *osc, hipStream_t st,
                              std::vector<int> &failed)
{
    const int nb = rq_words(idx->dim) * 8, groups = idx->rq_groups, sel_k = nominate_sel_k(k);
    const bool sampled = idx->n_tiles > 64;  // up to 4096 rows: every row is listed, the capacity holds them
    const int check = hook(kHookRabitqNomCheck) ? 1 : 0;
    const size_t before = failed.size();
    auto gemm = rabitq_nom_gemm_kernel;
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(gemm), hipFuncAttributeMaxDynamicSharedMemorySize, kRnLds));
    for (int64_t q0 = 0; q0 < nq; q0 += 4096) {
        const int cnt = static_cast<int>(std::min<int64_t>(4096, nq - q0));
        const int qpad = (cnt + kRnTile - 1) / kRnTile * kRnTile;
        const int slices = sampled ? rabitq_sample_slices(idx, cnt) : 0;
        const uint8_t *qc = qcodes + q0 * (nb + 4);
        ArenaCall ar(idx->ctx, st);
        const int i_qimg = ar.add(static_cast<size_t>(groups) * qpad * kRnStep);
        const int i_qn = ar.add(sizeof(float) * qpad), i_tau = ar.add(sizeof(float) * qpad);
        const int i_counts = ar.add(sizeof(int) * static_cast<size_t>(qpad) * kRnCountStride);
        const int i_cand = ar.add(sizeof(uint64_t) * static_cast<size_t>(qpad) * kRnCap);
        const int i_fail = ar.add(sizeof(int) * (static_cast<size_t>(cnt) + 1));  // + the pass's mismatch count
        const int i_partial = ar.add(sizeof(uint64_t) * static_cast<size_t>(cnt) * slices * sel_k);
        const int i_sid = ar.add(sizeof(uint32_t) * static_cast<size_t>(cnt) * sel_k), i_thr = ar.add(sizeof(float) * static_cast<size_t>(cnt) * sel_k);
        VG_TRY(ar.commit());
        int *counts = ar.get<int>(i_counts), *fail = ar.get<int>(i_fail);
        float *thr = sampled ? ar.get<float>(i_thr) : nullptr, *qn = ar.get<float>(i_qn), *tau = ar.get<float>(i_tau);
        uint8_t *qimg = ar.get<uint8_t>(i_qimg);
        uint64_t *cand = ar.get<uint64_t>(i_cand);
        VG_HIP(hipMemsetAsync(counts, 0, sizeof(int) * static_cast<size_t>(qpad) * kRnCountStride, st));
        VG_HIP(hipMemsetAsync(fail + cnt, 0, sizeof(int), st));
        if (sampled) VG_TRY(launch_rabitq_sample(idx, qc, cnt, sel_k, slices, ar.get<uint64_t>(i_partial), ar.get<uint32_t>(i_sid), thr, st));
        const int64_t prep = static_cast<int64_t>(qpad) * groups * 8;
        VG_LAUNCH(rabitq_nom_prep_kernel, dim3(static_cast<unsigned>((prep + 255) / 256)), dim3(256), 0, st, qc, nb, groups, cnt, qpad, thr, sel_k, qimg,
                  qn, tau);
        const int64_t tiles = ((idx->n + kRnTile - 1) / kRnTile) * (qpad / kRnTile);
        {
            ProfScope prof(idx->ctx, "rabitq_nom_gemm", st);
            VG_LAUNCH(gemm, dim3(static_cast<unsigned>(std::min<int64_t>(tiles, idx->ctx->compute_units))), dim3(kRnThreads), kRnLds, st,
                      idx->d_rq_tiles, idx->d_rq_norms, idx->n, idx->n_tiles, groups, qimg, qpad, qn, tau, rq_screen_invd(idx->dim), counts, cand);
        }
        {
            ProfScope prof(idx->ctx, "rabitq_nom_verify", st);
            VG_LAUNCH(rabitq_nom_verify_kernel, dim3(static_cast<unsigned>(cnt)), dim3(256), sizeof(uint64_t) * kRnCap, st, idx->d_rq_rows, qc, nb,
                      idx->dim, tau, counts, cand, k, oid + q0 * k, osc + q0 * k, fail, check, fail + cnt);
        }
        VG_TRY(failed_list(fail, cnt, q0, st, failed));
        if (check) {
            int bad = 0;
            VG_HIP(hipMemcpyAsync(&bad, fail + cnt, sizeof(int), hipMemcpyDeviceToHost, st));
            VG_HIP(hipStreamSynchronize(st));
            idx->rq_nom_mismatched += bad;
        }
    }
    idx->rq_nom_rescanned += static_cast<int64_t>(failed.size() - before);
    return VG_OK;
}

}  // namespace vg

VG_API int32_t vg_index_enable_rabitq_nomination(vg_index *idx, int32_t on, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_enable_rabitq_nomination: NULL index");
    VG_CHECK(idx->d_rq_tiles && idx->d_rq_rows, VG_ERR_NOT_READY, "vg_index_enable_rabitq_nomination: index has no RaBitQ codes");
    VG_TRY(vg::rabitq_nomination_drop(idx));
    if (!on) return VG_OK;
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    vg::DevTmp<int> flag;
    VG_TRY(flag.init(1, st));
    VG_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), st));
    VG_LAUNCH(vg::rabitq_nom_negative_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((idx->n + 255) / 256, 1024))), dim3(256), 0, st,
              idx->d_rq_norms, idx->n, flag.ptr);
    int neg = 0;
    VG_HIP(hipMemcpyAsync(&neg, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    idx->rq_nom_negative = neg != 0;
    idx->rq_nom_on = true;
    return VG_OK;
}

VG_API int32_t vg_index_rabitq_nomination_info(const vg_index *idx, int32_t *on, int64_t *held_bytes, int64_t *rescanned, int64_t *mismatched)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_rabitq_nomination_info: NULL index");
    if (on) *on = idx->rq_nom_on ? 1 : 0;
    if (held_bytes) *held_bytes = 0;  // the mode keeps nothing per row: its operands are the code tiles and norms
    if (rescanned) *rescanned = idx->rq_nom_on ? idx->rq_nom_rescanned : 0;
    if (mismatched) *mismatched = idx->rq_nom_on ? idx->rq_nom_mismatched : 0;
    return VG_OK;
}
