// k_binary_nominate.hip — vg_search_binary batches on the int8 matrix cores: the persistent 256 x 256 tile of k_rabitq_nominate.hip,
// changed in what binary codes make different.
//
// With the bits of a query and a row expanded to int8 (set: +1, clear: -1), s = sum s_q s_y = K - 2 h over the K = steps * 128 bit
// positions (the zero bits past dim are -1 on both sides and agree), and v_mfma_i32_32x32x32_i8 accumulates it exactly.  The score
// IS h, so — unlike the RaBitQ sibling — there is no float formula, no screen, no norms and no re-score:
//   1. threshold: the rows of every 64th 64-row tile scored by the scan kernel (launch_binary_sample, k_binary_search.hip);
//      tau_q = the h of the nominate_sel_k(k)-th best of them, "every row" when the index has no more than 64 tiles
//   2. the queries' bits expanded once into the GEMM's LDS image, tau_q turned into the bound on s (binary_nom_prep_kernel)
//   3. GEMM (binary_nom_gemm_kernel): the row fill reads the index's ROW-MAJOR codes — a K step is one 16-byte chunk of a row, two
//      lanes take its halves — and expands them in registers; no tiled copy exists.  The epilogue compares the int32 accumulator
//      with the query's integer bound (s >= K - 2 tau, i.e. h <= tau) and appends the FINAL key (make_key of float(h), the row)
//   4. select (binary_nom_select_kernel): the query's list sorted, the k best written, and the proof: the list did not overflow
//      (kBnCap keys) and holds at least k keys, or tau was "every row".  Every unlisted row has h > tau >= the k-th listed h.
//   5. a query whose proof failed goes through the scan and is counted (`rescanned`).  Rows at exactly h == tau that outnumber the
//      list (small dims, duplicate rows) overflow it: that ends in the scan's answer, never in a cut list.
// Nothing is resident and no result changes, so the path needs no enable call: vg_search_binary takes it for unfiltered batches
// of more than 128 queries, code bytes <= 1024, k <= 256, rows > k, from kBinaryNomMinPairs (k > 64: ...Paged) (query, row) pairs up.
#include <algorithm>
#include <climits>
#include <vector>

#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_nominate.hpp"
#include "vg_rabitq.hpp"
#include "vg_search.hpp"

namespace vg {

constexpr int kBnTile = 256;                 // queries and rows of a tile
constexpr int kBnThreads = 512;              // 8 waves: 2 (128 queries each) x 4 (64 rows each)
constexpr int kBnStep = 128;                 // int8 elements of a row or query per K step (16 code bytes)
constexpr int kBnImage = kBnTile * kBnStep;  // one operand's LDS image of a step: 32 KiB
constexpr int kBnLds = 4 * kBnImage;         // two steps of both images
constexpr int kBnCap = 4096;                 // keys kept per query
constexpr int kBnCountStride = 32;           // a query's counter every 128 bytes
constexpr int kBnMaxCodeBytes = 1024;
// Batches from this many (query, row) pairs up take the path (test hook VG_BINARY_NOM_ALWAYS: any number): the smallest products
// at which it beat the scan (tools/binary_search_time.py, dim 768; DESIGN.md "Exhaustive Hamming search").  129 x 100k: k = 100
// 0.326 against 1.066 ms (the scan runs a pass per page of 64 results), but k = 10 0.278 against 0.276 ms — no win, so up to one
// page the constant is the next product measured, 1024 x 100k (0.446 against 0.538 ms).
constexpr int64_t kBinaryNomMinPairs = 102400000;      // k <= 64
constexpr int64_t kBinaryNomMinPairsPaged = 12900000;  // k > 64

typedef int bn_i4 __attribute__((ext_vector_type(4)));
typedef int bn_i16 __attribute__((ext_vector_type(16)));

// byte offset of 16-byte chunk ch (0..7) of row r in a [256][128 B] image (the sibling's swizzle: 16 consecutive rows' reads of one
// chunk spread over the 16 slots of a 256-byte bank row)
__device__ __forceinline__ int bn_off(int r, int ch) { return r * kBnStep + ((ch ^ ((r >> 1) & 7)) << 4); }

// The queries' LDS image [step][qpad][128 B] and their bound on s.  Queries from cnt to qpad: no bits, a bound no s reaches.
// thr: the sample's sel_k best scores per query (null: every row is listed).  One thread per (query, step, chunk).
__global__ __launch_bounds__(256) void binary_nom_prep_kernel(const uint8_t *__restrict__ qcodes, int cb, int steps, int cnt, int qpad,
                                                              const float *__restrict__ thr, int sel_k, uint8_t *__restrict__ qimg,
                                                              int *__restrict__ smin)
{
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (gid >= static_cast<int64_t>(qpad) * steps * 8) return;
    const int ch = static_cast<int>(gid & 7);
    const int q = static_cast<int>((gid >> 3) % qpad);
    const int s = static_cast<int>((gid >> 3) / qpad);
    uint32_t bits = 0;
    const int at = s * 16 + ch * 2;
    if (q < cnt && at < cb) bits = qcodes[static_cast<int64_t>(q) * cb + at] | (static_cast<uint32_t>(qcodes[static_cast<int64_t>(q) * cb + at + 1]) << 8);
    *reinterpret_cast<uint4 *>(qimg + (static_cast<int64_t>(s) * qpad + (q & ~255)) * kBnStep + bn_off(q & 255, ch)) = rn_expand16(bits);
    if (s == 0 && ch == 0) {
        int bound = INT_MAX;  // (a padding query)
        if (q < cnt) {
            const float t = thr ? thr[static_cast<int64_t>(q) * sel_k + (sel_k - 1)] : INFINITY;
            bound = t == INFINITY ? INT_MIN : steps * 128 - 2 * static_cast<int>(t);  // h <= tau  <=>  s >= K - 2 tau
        }
        smin[q] = bound;
    }
}

// The GEMM: the sibling's schedule (workgroup b takes tiles b, b + gridDim.x, ... of the (row tile, query tile) grid, query tiles
// innermost; per K step both operands' 128 int8 in LDS, two buffers, one barrier a step; wave (wq, wr) multiplies rows wr * 64 ..
// + 63 by queries wq * 128 .. + 127, result register r of lane l: query l & 31, row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the block).
// The fill: thread (fr, fhalf) reads 8 bytes of row fr's 16-byte chunk `s` from the row-major codes (cb a row) and expands them.
__global__ __launch_bounds__(kBnThreads) void binary_nom_gemm_kernel(const uint8_t *__restrict__ codes, int64_t n, int cb, int steps,
                                                                     const uint8_t *__restrict__ qimg, int qpad, const int *__restrict__ smin,
                                                                     int *__restrict__ counts, uint64_t *__restrict__ cand)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bn_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave & 1, wr = wave >> 1;
    const int n_qt = qpad / kBnTile;
    const int64_t total = ((n + kBnTile - 1) / kBnTile) * n_qt;
    const int fr = tid & 255, fhalf = tid >> 8;
    const int ksum = steps * 128;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int q0 = static_cast<int>(t % n_qt) * kBnTile;
        const int64_t row0 = (t / n_qt) * kBnTile;
        uint4 qreg0, qreg1, qreg2, qreg3;
        uint2 rreg;
        const int64_t frow = row0 + fr;
        auto load = [&](int s) {
            const uint4 *src = reinterpret_cast<const uint4 *>(qimg + (static_cast<int64_t>(s) * qpad + q0) * kBnStep);
            qreg0 = src[tid];
            qreg1 = src[kBnThreads + tid];
            qreg2 = src[2 * kBnThreads + tid];
            qreg3 = src[3 * kBnThreads + tid];
            rreg = make_uint2(0u, 0u);
            const int at = s * 16 + fhalf * 8;  // (cb is a multiple of 8: a half lies inside the row or past it)
            if (frow < n && at < cb) rreg = *reinterpret_cast<const uint2 *>(codes + frow * cb + at);
        };
        auto store = [&](int buf) {
            unsigned char *qb = bn_smem + buf * 2 * kBnImage, *rb = qb + kBnImage;
            reinterpret_cast<uint4 *>(qb)[tid] = qreg0;
            reinterpret_cast<uint4 *>(qb)[kBnThreads + tid] = qreg1;
            reinterpret_cast<uint4 *>(qb)[2 * kBnThreads + tid] = qreg2;
            reinterpret_cast<uint4 *>(qb)[3 * kBnThreads + tid] = qreg3;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t w = j < 2 ? rreg.x : rreg.y;
                *reinterpret_cast<uint4 *>(rb + bn_off(fr, fhalf * 4 + j)) = rn_expand16((w >> (16 * (j & 1))) & 0xFFFFu);
            }
        };
        bn_i16 acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 4; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[a][b][r] = 0;
        __syncthreads();  // the previous tile's last step is read
        load(0);
        store(0);
        __syncthreads();
        for (int s = 0; s < steps; s++) {
            const bool more = s + 1 < steps;
            if (more) load(s + 1);
            const unsigned char *qb = bn_smem + (s & 1) * 2 * kBnImage, *rb = qb + kBnImage;
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const int ch = 2 * kk + (lane >> 5);
                bn_i4 a[2], b[4];
#pragma unroll
                for (int i = 0; i < 2; i++) a[i] = *reinterpret_cast<const bn_i4 *>(rb + bn_off(wr * 64 + i * 32 + (lane & 31), ch));
#pragma unroll
                for (int i = 0; i < 4; i++) b[i] = *reinterpret_cast<const bn_i4 *>(qb + bn_off(wq * 128 + i * 32 + (lane & 31), ch));
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
            }
            if (more) store((s + 1) & 1);
            __syncthreads();
        }
        // the epilogue, integers only: s >= the query's bound, the row exists -> the final key joins the query's list
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int q = q0 + wq * 128 + j * 32 + (lane & 31);
            const int bound = smin[q];
#pragma unroll
            for (int i = 0; i < 2; i++) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int sv = acc[i][j][r];
                    const int64_t row = row0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (sv >= bound && row < n) {
                        const int pos = atomicAdd(counts + static_cast<int64_t>(q) * kBnCountStride, 1);
                        if (pos < kBnCap)
                            cand[static_cast<int64_t>(q) * kBnCap + pos] = make_key(static_cast<float>((ksum - sv) >> 1), static_cast<uint32_t>(row), false);
                    }
                }
            }
        }
    }
}

// Per query: the list sorted, the k best written, and the proof (the head of this file).  every_row: no threshold was sampled.
__global__ __launch_bounds__(256) void binary_nom_select_kernel(const int *__restrict__ counts, const uint64_t *__restrict__ cand, int k,
                                                                int every_row, uint32_t *__restrict__ ids, float *__restrict__ scores,
                                                                int *__restrict__ fail)
{
    extern __shared__ uint64_t bn_sort[];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const int total = counts[q * kBnCountStride];
    const int cnt = total < kBnCap ? total : kBnCap;
    int n2 = 64;
    while (n2 < cnt) n2 <<= 1;
    for (int i = tid; i < n2; i += 256) bn_sort[i] = i < cnt ? cand[q * kBnCap + i] : kKeyMax;
    __syncthreads();
    bitonic_sort_lds(bn_sort, n2, tid, 256);
    for (int i = tid; i < k; i += 256) {
        const uint64_t e = i < n2 ? bn_sort[i] : kKeyMax;
        ids[q * k + i] = e == kKeyMax ? VG_INVALID_ID : key_row(e);
        scores[q * k + i] = e == kKeyMax ? INFINITY : key_score(e, false);
    }
    if (tid == 0) fail[q] = total <= kBnCap && (every_row || total >= k) ? 0 : 1;
}

// a small kernel in place of a memset (the counters of a pass)
__global__ void binary_nom_clear_kernel(int *__restrict__ p, int64_t count)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < count) p[i] = 0;
}

bool binary_nomination_applies(const vg_index *idx, int64_t nq, int k, const uint8_t *mask)
{
    if (hook(kHookBinaryNoNom) || mask || nq <= 128 || k > kNomMaxK || idx->n <= k) return false;
    if (vg_binary_code_bytes(idx->dim) > kBnMaxCodeBytes) return false;
    return nq * idx->n >= (k > 64 ? kBinaryNomMinPairsPaged : kBinaryNomMinPairs) || hook(kHookBinaryNomAlways);
}

int32_t binary_nominated_pass(vg_index *idx, const float *q, int64_t nq, int k, uint32_t *oid, float *osc, hipStream_t st, std::vector<int> &failed)
{
    const int cb = static_cast<int>(vg_binary_code_bytes(idx->dim)), steps = (cb + 15) / 16, sel_k = nominate_sel_k(k);
    const bool sampled = (idx->n + 63) / 64 > 64;  // up to 4096 rows: every row is listed, the capacity holds them
    const size_t before = failed.size();
    auto gemm = binary_nom_gemm_kernel;
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(gemm), hipFuncAttributeMaxDynamicSharedMemorySize, kBnLds));
    for (int64_t q0 = 0; q0 < nq; q0 += 4096) {
        const int cnt = static_cast<int>(std::min<int64_t>(4096, nq - q0));
        const int qpad = (cnt + kBnTile - 1) / kBnTile * kBnTile;
        const int slices = sampled ? binary_sample_slices(idx, cnt) : 0;
        ArenaCall ar(idx->ctx, st);
        const int i_qc = ar.add(static_cast<size_t>(cnt) * cb);
        const int i_qimg = ar.add(static_cast<size_t>(steps) * qpad * kBnStep);
        const int i_smin = ar.add(sizeof(int) * qpad);
        const int i_counts = ar.add(sizeof(int) * static_cast<size_t>(qpad) * kBnCountStride);
        const int i_cand = ar.add(sizeof(uint64_t) * static_cast<size_t>(qpad) * kBnCap);
        const int i_fail = ar.add(sizeof(int) * static_cast<size_t>(cnt));
        const int i_partial = ar.add(sizeof(uint64_t) * static_cast<size_t>(cnt) * slices * sel_k);
        const int i_sid = ar.add(sizeof(uint32_t) * static_cast<size_t>(cnt) * sel_k), i_thr = ar.add(sizeof(float) * static_cast<size_t>(cnt) * sel_k);
        VG_TRY(ar.commit());
        uint8_t *qc = ar.get<uint8_t>(i_qc), *qimg = ar.get<uint8_t>(i_qimg);
        int *counts = ar.get<int>(i_counts), *fail = ar.get<int>(i_fail), *smin = ar.get<int>(i_smin);
        float *thr = sampled ? ar.get<float>(i_thr) : nullptr;
        uint64_t *cand = ar.get<uint64_t>(i_cand);
        VG_TRY(launch_binary_encode(q + q0 * idx->dim, cnt, idx->dim, idx->bin_threshold, qc, st));
        const int64_t ncount = static_cast<int64_t>(qpad) * kBnCountStride;
        VG_LAUNCH(binary_nom_clear_kernel, dim3(static_cast<unsigned>((ncount + 255) / 256)), dim3(256), 0, st, counts, ncount);
        if (sampled)
            VG_TRY(launch_binary_sample(idx, reinterpret_cast<const uint64_t *>(qc), cnt, sel_k, slices, ar.get<uint64_t>(i_partial),
                                        ar.get<uint32_t>(i_sid), thr, st));
        const int64_t prep = static_cast<int64_t>(qpad) * steps * 8;
        VG_LAUNCH(binary_nom_prep_kernel, dim3(static_cast<unsigned>((prep + 255) / 256)), dim3(256), 0, st, qc, cb, steps, cnt, qpad, thr, sel_k, qimg,
                  smin);
        const int64_t tiles = ((idx->n + kBnTile - 1) / kBnTile) * (qpad / kBnTile);
        {
            ProfScope prof(idx->ctx, "binary_nom_gemm", st);
            VG_LAUNCH(gemm, dim3(static_cast<unsigned>(std::min<int64_t>(tiles, idx->ctx->compute_units))), dim3(kBnThreads), kBnLds, st,
                      idx->d_bin_rows, idx->n, cb, steps, qimg, qpad, smin, counts, cand);
        }
        {
            ProfScope prof(idx->ctx, "binary_nom_select", st);
            VG_LAUNCH(binary_nom_select_kernel, dim3(static_cast<unsigned>(cnt)), dim3(256), sizeof(uint64_t) * kBnCap, st, counts, cand, k,
                      sampled ? 0 : 1, oid + q0 * k, osc + q0 * k, fail);
        }
        VG_TRY(failed_list(fail, cnt, q0, st, failed));
    }
    idx->bin_nominated += nq;
    idx->bin_rescanned += static_cast<int64_t>(failed.size() - before);
    return VG_OK;
}

}  // namespace vg
