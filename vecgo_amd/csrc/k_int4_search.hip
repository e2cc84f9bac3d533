// k_int4_search.hip — vg_search_int4: the exhaustive top-k search over an index's INT4 codes (vg_index_set_int4_codes).  The
// reference scores INT4 codes node by node in the DiskANN walk (diskann/segment.go:558-565: Int4Quantizer.L2Distance,
// int4.go:136-147 = int4L2DistancePrecomputedAvx512, int4_avx512.c:127-189); the scan over all rows is this library's: the
// candidate stage of a rerank pipeline at 4 bits a dimension, the answer to a selective filter, and the walk's ground truth in
// the walk's own arithmetic — every score has the bits vg_int4_l2_distance_batch(precomputed = 1) and vg_search_vamana kind 3
// give the row.  Nothing new is resident: the kernels read the index's row-major codes.
#include <algorithm>

#include "vg_cand_replay.hpp"
#include "vg_device.hpp"
#include "vg_int4_plan.hpp"
#include "vg_int4_scan.hpp"
#include "vg_internal.hpp"
#include "vg_scan_slices.hpp"
#include "vg_search.hpp"

namespace vg {

constexpr int kI4sWaves = 4;  // waves (64-row tiles in flight) of the pair-table, lane-per-row and multi-query workgroups
constexpr int kI4sQB = 8;     // queries a multi-query workgroup carries over its slice: 8 x 8 packed accumulators + 16 decoded
                              // pairs + 8 key lists per lane stay in registers (236 VGPRs, no scratch: profiles/kernel_resources.txt)
// From how many queries a batch takes the multi-query kernel (dim % 32 == 0).  Measured (MI355X, tools/int4_search_time.py, dim 768,
// k = 10, ms per call, multi-query kernel against nq x the one-query search): 1M rows — 3 queries 0.582 / 0.393, 4: 0.599 / 0.524,
// 5: 0.620 / 0.655, 8: 0.677 / 1.047; 100k rows — 3: 0.167 / 0.146, 4: 0.175 / 0.195, 5: 0.182 / 0.244.  It wins from 5 at both.
constexpr int64_t kI4sMqMinQueries = 5;
constexpr int kI4sSmallGrid = 2;  // workgroups / slices under the test hook VG_INT4_SEARCH_SMALL_GRID

// The 64 keys of a wave, one per lane, sorted ascending across the lanes (bitonic: 21 compare-exchange steps through lane
// shuffles): lane i ends with the i-th smallest.  Equal keys (kKeyMax) may sit in any of their places.
__device__ __forceinline__ uint64_t wave_sort_keys(uint64_t key, int lane)
{
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const uint32_t olo = __shfl_xor(static_cast<uint32_t>(key), stride);
            const uint32_t ohi = __shfl_xor(static_cast<uint32_t>(key >> 32), stride);
            const uint64_t other = (static_cast<uint64_t>(ohi) << 32) | olo;
            const bool up = (lane & size) == 0;         // this lane's block of `size` ascends (the last step: all 64)
            const bool lower = (lane & stride) == 0;    // the lower lane of the pair
            const bool take_min = lower == up;
            const bool other_less = other < key;
            key = (take_min == other_less) ? other : key;
        }
    }
    return key;
}

// The search's epilogue of the shared row loops (vg_int4_scan.hpp): a row that takes part and may still enter (a float test
// against the score of the wave's k-th key first) offers its key to the wave's top-k.
struct Int4OfferEpi {
    WaveTopK tk;
    float tau_d;  // score of the k-th key (+Inf until k keys were seen)
    int64_t n;
    const uint8_t *__restrict__ mask;  // the query's row filter, or null
    uint64_t floor_key;                // paged results: only keys after the previous page's last one
    bool paged;
    bool empty;  // (uniform) no key has been kept yet
    __device__ __forceinline__ void init(int k, int64_t n_, const uint8_t *mask_, const uint64_t *min_keys, int64_t q)
    {
        tk.init(k);
        tau_d = INFINITY;
        empty = true;
        n = n_;
        mask = mask_;
        paged = min_keys != nullptr;
        floor_key = paged ? min_keys[q] : 0;
    }
    __device__ __forceinline__ bool live_tile(int64_t tile, int lane) const
    {
        if (mask == nullptr) return true;
        const int64_t r = tile * 64 + lane;
        return __ballot(r < n && mask_bit(mask, r)) != 0;
    }
    __device__ __forceinline__ void row(int64_t row0, int lane, float total)
    {
        const int64_t r = row0 + lane;
        const bool live = r < n && mask_bit(mask, r);
        if (__ballot(live && total <= tau_d)) {
            uint64_t key = live ? make_key(total, static_cast<uint32_t>(r), false) : kKeyMax;
            if (paged && key <= floor_key) key = kKeyMax;
            if (empty) {
                // the wave's first tile: its 64 keys sorted ARE the list (WaveTopK would insert them one by one, some 30 rounds
                // of a dozen instructions — as much work as scoring a tile, and a wave of a one-query scan over 1M rows sees
                // only 5 tiles)
                tk.list = wave_sort_keys(key, lane);
                tk.tau = readlane_u64(tk.list, tk.k - 1);
                empty = false;
            } else {
                tk.offer(key, lane);
            }
            tau_d = tk.tau == kKeyMax ? INFINITY : key_score(tk.tau, false);
        }
    }
};

// One query per blockIdx.y, the pair-table form (dim % 64 == 0): int4_scan_kernel's row loop, the tiles DEALT round-robin over
// the workgroups (trip i of workgroup s, wave w = tile (i * slices + s) * waves + w: the chip streams one moving window of the
// codes), the workgroup's k best to partial[(q * slices + s) * k].
__global__ __launch_bounds__(kI4sWaves * 64) void int4_search_pair_kernel(const float *__restrict__ queries, const uint8_t *__restrict__ codes,
                                                                          int64_t n, int dim, const float *__restrict__ mins,
                                                                          const float *__restrict__ diff, const uint8_t *__restrict__ mask,
                                                                          int64_t mask_stride, int k, uint64_t *__restrict__ partial,
                                                                          const uint64_t *__restrict__ min_keys)
{
    __shared__ vg_f2v pairs[256];
    __shared__ __attribute__((aligned(16))) unsigned char stage_all[kI4sWaves][64 * kI4Stride];
    __shared__ uint64_t lists[kI4sWaves * 64];
    __shared__ int valid[kI4sWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.y;
    const int s = blockIdx.x, slices = gridDim.x;
    int4_scan_fill_pairs<true>(pairs, tid);
    __syncthreads();
    Int4OfferEpi epi;
    epi.init(k, n, mask ? mask + q * mask_stride : nullptr, min_keys, q);
    const float *query = queries + q * dim;
    const int64_t n_tiles = (n + 63) / 64;
    for (int64_t tile = static_cast<int64_t>(s) * kI4sWaves + wave; tile < n_tiles; tile += static_cast<int64_t>(slices) * kI4sWaves) {
        if (!epi.live_tile(tile, lane)) continue;  // (uniform) a tile the filter drops whole is not read
        int4_pair_tile<true>(query, codes, n, dim, mins, diff, pairs, stage_all[wave], lane, tile * 64, epi);
    }
    wg_rank_merge<kI4sWaves>(epi.tk, lists, valid, wave, lane, tid, k, partial + (q * slices + s) * k);
}

// One query per blockIdx.y, the LDS table form (dim % 256 == 0, dim <= 1024): int4_scan_tab_kernel's persistent waves (their
// tiles are dealt round-robin already), launch shape from int4_scan_plan.  The merge's lists take the table's place in LDS.
__global__ __launch_bounds__(kI4TabWaves * 64) void int4_search_tab_kernel(const float *__restrict__ queries, const uint8_t *__restrict__ codes,
                                                                           int64_t n, int dim, const float *__restrict__ mins,
                                                                           const float *__restrict__ diff, const uint8_t *__restrict__ mask,
                                                                           int64_t mask_stride, int k, uint64_t *__restrict__ partial,
                                                                           const uint64_t *__restrict__ min_keys)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char i4smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const int64_t q = blockIdx.y;
    const int s = blockIdx.x, slices = gridDim.x;
    Int4OfferEpi epi;
    epi.init(k, n, mask ? mask + q * mask_stride : nullptr, min_keys, q);
    int4_tab_scan<true>(i4smem, queries + q * dim, codes, n, dim, mins, diff, nullptr, epi);
    __syncthreads();  // every wave is done with the table (at least 16 KiB: dim >= 256)
    uint64_t *lists = reinterpret_cast<uint64_t *>(i4smem);
    int *valid = reinterpret_cast<int *>(lists + kI4TabWaves * 64);
    // the merge is written for kI4TabWaves lists; a workgroup of fewer waves (dim 1024: 10) leaves the others empty
    for (int i = waves * 64 + tid; i < kI4TabWaves * 64; i += blockDim.x) lists[i] = kKeyMax;
    if (tid < kI4TabWaves - waves) valid[waves + tid] = 0;
    wg_rank_merge<kI4TabWaves>(epi.tk, lists, valid, wave, lane, tid, k, partial + (q * slices + s) * k);
}

// One query per blockIdx.y, any dim: a lane per row with int4_l2_precomputed (the quantizer's dim x 16 table in memory), 64-row
// tiles dealt as above.
__global__ __launch_bounds__(kI4sWaves * 64) void int4_search_row_kernel(const float *__restrict__ queries, const uint8_t *__restrict__ codes,
                                                                         int64_t n, int dim, const float *__restrict__ table,
                                                                         const uint8_t *__restrict__ mask, int64_t mask_stride, int k,
                                                                         uint64_t *__restrict__ partial, const uint64_t *__restrict__ min_keys)
{
    __shared__ uint64_t lists[kI4sWaves * 64];
    __shared__ int valid[kI4sWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.y;
    const int s = blockIdx.x, slices = gridDim.x;
    Int4OfferEpi epi;
    epi.init(k, n, mask ? mask + q * mask_stride : nullptr, min_keys, q);
    const float *query = queries + q * dim;
    const int64_t n_tiles = (n + 63) / 64, cs = (dim + 1) / 2;
    for (int64_t tile = static_cast<int64_t>(s) * kI4sWaves + wave; tile < n_tiles; tile += static_cast<int64_t>(slices) * kI4sWaves) {
        if (!epi.live_tile(tile, lane)) continue;
        const int64_t r = tile * 64 + lane;
        const float total = int4_l2_precomputed(query, codes + (r < n ? r : n - 1) * cs, dim, table);
        epi.row(tile * 64, lane, total);
    }
    wg_rank_merge<kI4sWaves>(epi.tk, lists, valid, wave, lane, tid, k, partial + (q * slices + s) * k);
}

// A BATCH of queries (dim % 32 == 0).  Run one query at a time every query streams and DECODES all the codes again; here a
// workgroup takes QB queries over its slice of the tiles.  A lane owns a row: per 32-dimension block it loads the row's 16 code
// bytes, decodes them ONCE into 16 packed pairs (a * diff + min, unfused, a from the 256-entry pair table in LDS — int4_l2_direct's
// arithmetic, the table's own: int4.go:152-163), and runs each of the QB queries over those values: per query and pair one packed
// subtract and one packed fma(d, d, sum[p]) with the query's values wave-uniform (LDS broadcast reads of the block's staged queries;
// as scalar loads the 8 x 32 values of a block did not fit the scalar registers and every refill was a round trip the wave waited out).  Each query has the 8 packed
// accumulators of int4L2DistancePrecomputedAvx512 (both 16-element halves of a 32-block feed sum[] in order) and its own
// WaveTopK.  Bound by the vector ALU: about one packed instruction pair per two dimensions and (query, row); the decode and the
// code bytes are shared by the QB queries.  Block order as in rabitq_scan_mq_kernel: the query blocks of one slice run on one
// XCD and share the slice in its L2 (plain loads: the codes are read again by the next query block).  A per-query filter turns
// the key into kKeyMax; a batch filter (mask_stride 0) skips a tile none of whose rows it keeps.
template <int QB>
__global__ __launch_bounds__(kI4sWaves * 64) void int4_search_mq_kernel(const float *__restrict__ queries, const uint8_t *__restrict__ codes,
                                                                        int64_t n, int64_t n_tiles, int dim, const float *__restrict__ mins,
                                                                        const float *__restrict__ diff, const uint8_t *__restrict__ mask,
                                                                        int64_t mask_stride, int slices, int nq, int k,
                                                                        uint64_t *__restrict__ partial, const uint64_t *__restrict__ min_keys)
{
    extern __shared__ __attribute__((aligned(16))) float i4q_smem[];  // the block's QB queries, [QB][dim]
    __shared__ vg_f2v pairs[256];
    __shared__ uint64_t lists[kI4sWaves * 64];
    __shared__ int valid[kI4sWaves];
    const int ng = (nq + QB - 1) / QB;
    const int b = blockIdx.x;
    int qg, s;
    if ((slices & 7) == 0) {
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
    int4_fill_pairs(pairs, tid, kI4sWaves * 64);
    for (int e = tid; e < QB * dim; e += kI4sWaves * 64) {  // a block's missing queries repeat its last one and are not merged
        const int qi = e / dim, j = e - qi * dim;
        i4q_smem[e] = queries[static_cast<int64_t>(q0 + (qi < cnt ? qi : cnt - 1)) * dim + j];
    }
    __syncthreads();
    const uint8_t *mq[QB];
    WaveTopK tk[QB];
    float tau_d[QB];
#pragma unroll
    for (int qi = 0; qi < QB; qi++) {
        const int64_t q = q0 + (qi < cnt ? qi : cnt - 1);
        mq[qi] = mask ? mask + q * mask_stride : nullptr;
        tk[qi].init(k);
        tau_d[qi] = INFINITY;
    }
    const bool batch_mask = mask != nullptr && (mask_stride == 0 || nq == 1);
    const int row_bytes = dim >> 1;
    for (int64_t tile = t0 + wave; tile < t1; tile += kI4sWaves) {
        const int64_t row = tile * 64 + lane;
        const bool inb = row < n;
        const bool keep = inb && (!batch_mask || mask_bit(mask, row));  // a batch filter's bit: read once for the QB queries
        if (batch_mask && !__ballot(keep)) continue;                    // (uniform) not read
        const uint8_t *cp = codes + (inb ? row : n - 1) * row_bytes;
        vg_f2v sum[QB][8];
#pragma unroll
        for (int qi = 0; qi < QB; qi++)
#pragma unroll
            for (int p = 0; p < 8; p++) sum[qi][p] = vg_f2v{0.0f, 0.0f};
        uint4 c = *reinterpret_cast<const uint4 *>(cp);
        for (int i = 0; i < dim; i += 32) {
            const int inext = i + 32 < dim ? i + 32 : i;  // (the last block again: unused)
            const uint4 cn = *reinterpret_cast<const uint4 *>(cp + (inext >> 1));
            const uint32_t w[4] = {c.x, c.y, c.z, c.w};
            vg_f2v t[16];
#pragma unroll
            for (int byte = 0; byte < 16; byte++) {
                const uint32_t bb = (w[byte >> 2] >> (8 * (byte & 3))) & 0xFFu;
                const int j = i + 2 * byte;
                const vg_f2v a = pairs[bb];
                const vg_f2v df = *reinterpret_cast<const vg_f2v *>(diff + j);
                const vg_f2v mn = *reinterpret_cast<const vg_f2v *>(mins + j);
                vg_f2v v = a * df;
                v = v + mn;
                t[byte] = v;
            }
#pragma unroll
            for (int qi = 0; qi < QB; qi++) {
                const float *qs = i4q_smem + qi * dim + i;  // (uniform address: one broadcast read serves the wave)
#pragma unroll
                for (int g = 0; g < 8; g++) {  // bytes 0..7: the first 16-element half, 8..15 the second, into sum[byte & 7]
                    const vg_f4v q4 = *reinterpret_cast<const vg_f4v *>(qs + 4 * g);
                    const vg_f2v d0 = vg_f2v{q4.x, q4.y} - t[2 * g];
                    const vg_f2v d1 = vg_f2v{q4.z, q4.w} - t[2 * g + 1];
                    sum[qi][(2 * g) & 7] = __builtin_elementwise_fma(d0, d0, sum[qi][(2 * g) & 7]);
                    sum[qi][(2 * g + 1) & 7] = __builtin_elementwise_fma(d1, d1, sum[qi][(2 * g + 1) & 7]);
                }
            }
            c = cn;
        }
#pragma unroll
        for (int qi = 0; qi < QB; qi++) {
            if (qi < cnt) {
                float s16[16];
#pragma unroll
                for (int p = 0; p < 8; p++) {
                    s16[2 * p] = sum[qi][p].x;
                    s16[2 * p + 1] = sum[qi][p].y;
                }
                const float total = reduce16_regs(s16);
                const bool live = batch_mask ? keep : inb && mask_bit(mq[qi], row);
                if (__ballot(live && total <= tau_d[qi])) {
                    uint64_t key = live ? make_key(total, static_cast<uint32_t>(row), false) : kKeyMax;
                    if (min_keys && key <= min_keys[q0 + qi]) key = kKeyMax;
                    tk[qi].offer(key, lane);
                    tau_d[qi] = tk[qi].tau == kKeyMax ? INFINITY : key_score(tk[qi].tau, false);
                }
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < QB; qi++) {
        if (qi < cnt) {
            wg_rank_merge<kI4sWaves>(tk[qi], lists, valid, wave, lane, tid, k, partial + (static_cast<int64_t>(q0 + qi) * slices + s) * k);
            __syncthreads();
        }
    }
}

// vg_cand_replay.hpp's scorer for the INT4 scan: Int4Quantizer.L2Distance of a row (int4_l2_precomputed, a row per thread).  A
// NaN: a non-finite query value, min or diff (the lookup table is float(v) / 15 * diff + min of them), or magnitudes whose squared
// differences overflow.
struct Int4Scorer {
    const uint8_t *rows;  // n * ceil(dim / 2)
    const float *table, *mn, *diff;
    int dim;
    __device__ bool risk(int64_t, const float *q, int tid) const
    {
        __shared__ int flag;
        __shared__ int vm_bits;
        if (tid == 0) vm_bits = 0;
        __syncthreads();
        bool bad = false;
        float vm = 0.0f;  // the largest |decoded value| there can be
        for (int j = tid; j < dim; j += kReplayThreads) {
            bad = bad || !is_finite_f32(mn[j]) || !is_finite_f32(diff[j]) || !is_finite_f32(q[j]);
            vm = fmaxf(vm, fabsf(mn[j]) + fabsf(diff[j]));
        }
        if (vm == vm) atomicMax(&vm_bits, __float_as_int(vm));  // (non-negative floats order like their bits; +Inf included)
        __syncthreads();
        vm = __int_as_float(vm_bits);
        bad = bad || !is_finite_f32(vm);
        for (int j = tid; j < dim; j += kReplayThreads)
            bad = bad || !(score_bound(fabsf(q[j]), vm, false) * static_cast<float>(dim) < 1e38f);
        return block_any(bad, &flag, tid);
    }
    __device__ void prepare(int64_t, const float *, int) const {}
    __device__ void score_chunk(int64_t, const float *q, int64_t row0, int64_t n, int tid, float *out) const
    {
        const int64_t row = row0 + tid;
        if (row >= n) return;
        out[tid] = int4_l2_precomputed(q, rows + row * ((dim + 1) / 2), dim, table);
    }
};

// the scan of nq queries (device buffers): path, launch shape, pages beyond 64 results, merge
static int32_t int4_scan_batch(vg_index *idx, const float *q, int64_t nq, int k, const uint8_t *mask, int64_t mask_stride, uint32_t *oid,
                               float *osc, hipStream_t st)
{
    const int dim = idx->dim, cus = idx->ctx->compute_units;
    const int64_t n = idx->n, n_tiles = (n + 63) / 64;
    const bool small = hook(kHookInt4SearchSmallGrid);
    enum { kMq, kTab, kPair, kRow } path;
    // vg_int4_plan.hpp's rules for one query (the index's codes are 16-byte aligned: hipMalloc, rows of dim / 2 bytes)
    const size_t mq_lds = sizeof(float) * kI4sQB * static_cast<size_t>(dim);  // the query block in LDS: dim <= 4096
    if (dim % 32 == 0 && nq >= kI4sMqMinQueries && mq_lds <= 128 * 1024)
        path = kMq;
    else if (dim % 64 != 0)
        path = kRow;
    else
        path = dim % 256 == 0 && dim <= kI4TabMaxDim ? kTab : kPair;
    const Int4ScanPlan plan = int4_scan_plan(dim, true, n, cus, small);
    int slices;
    if (path == kTab)
        slices = static_cast<int>(plan.blocks);
    else if (small)
        slices = kI4sSmallGrid;
    else
        slices = scan_slices(path == kMq ? (nq + kI4sQB - 1) / kI4sQB : nq, (n_tiles + kI4sWaves - 1) / kI4sWaves, cus, 4);
    ArenaCall ar(idx->ctx, st);
    PagedTopK pages;  // a wave keeps 64 keys: k > 64 comes in pages of 64, one scan per page
    pages.add(ar, nq, k, slices);
    VG_TRY(ar.commit());
    if (path == kTab)
        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(int4_search_tab_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(plan.lds)));
    if (path == kMq && mq_lds > 32 * 1024)
        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(int4_search_mq_kernel<kI4sQB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(mq_lds)));
    return pages.run(ar, slices, false, oid, osc, st, [&](int kk, uint64_t *partial, const uint64_t *floor) -> int32_t {
        if (path == kMq) {
            const int64_t max_q = (1ll << 30) / slices * kI4sQB;  // whole query blocks per launch
            for (int64_t q0 = 0; q0 < nq; q0 += max_q) {
                const int64_t cnt = std::min<int64_t>(nq - q0, max_q);
                const int64_t ng = (cnt + kI4sQB - 1) / kI4sQB;
                ProfScope prof(idx->ctx, "int4_search_mq", st);
                VG_LAUNCH(int4_search_mq_kernel<kI4sQB>, dim3(static_cast<unsigned>(ng * slices)), dim3(kI4sWaves * 64), mq_lds, st, q + q0 * dim,
                          idx->d_int4_rows, n, n_tiles, dim, idx->int4_min, idx->int4_diff, mask ? mask + q0 * mask_stride : nullptr, mask_stride,
                          slices, static_cast<int>(cnt), kk, partial + q0 * slices * kk, floor ? floor + q0 : nullptr);
            }
            return VG_OK;
        }
        for (int64_t q0 = 0; q0 < nq; q0 += 65535) {  // a query per blockIdx.y
            const int64_t cnt = std::min<int64_t>(nq - q0, 65535);
            const dim3 grid(static_cast<unsigned>(slices), static_cast<unsigned>(cnt));
            const float *qq = q + q0 * dim;
            const uint8_t *mm = mask ? mask + q0 * mask_stride : nullptr;
            uint64_t *pp = partial + q0 * slices * kk;
            const uint64_t *ff = floor ? floor + q0 : nullptr;
            ProfScope prof(idx->ctx, path == kRow ? "int4_search_row" : "int4_search_one", st);
            if (path == kTab)
                VG_LAUNCH(int4_search_tab_kernel, grid, dim3(plan.waves * 64), static_cast<size_t>(plan.lds), st, qq, idx->d_int4_rows, n, dim,
                          idx->int4_min, idx->int4_diff, mm, mask_stride, kk, pp, ff);
            else if (path == kPair)
                VG_LAUNCH(int4_search_pair_kernel, grid, dim3(kI4sWaves * 64), 0, st, qq, idx->d_int4_rows, n, dim, idx->int4_min,
                          idx->int4_diff, mm, mask_stride, kk, pp, ff);
            else
                VG_LAUNCH(int4_search_row_kernel, grid, dim3(kI4sWaves * 64), 0, st, qq, idx->d_int4_rows, n, dim, idx->int4_table, mm,
                          mask_stride, kk, pp, ff);
        }
        return VG_OK;
    });
}

}  // namespace vg

VG_API int32_t vg_search_int4(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask, int64_t mask_stride,
                              uint32_t *ids, float *scores, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_search_int4: NULL index");
    VG_CHECK(nq >= 0 && k >= 0, VG_ERR_INVALID_ARG, "vg_search_int4: negative nq or k");
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(idx->n == 0 || idx->d_int4_rows, VG_ERR_NOT_READY, "vg_search_int4: index has no INT4 codes");
    VG_CHECK(queries && ids && scores, VG_ERR_INVALID_ARG, "vg_search_int4: NULL buffer");
    VG_CHECK(k <= 512, VG_ERR_UNSUPPORTED, "vg_search_int4: k=%d exceeds 512", k);
    if (nq > 1) VG_CHECK_MASK_STRIDE("vg_search_int4", mask, mask_stride, idx->n);
    vg::SearchIO io;
    VG_TRY(io.init(idx->ctx, stream, queries, static_cast<size_t>(nq) * idx->dim, ids, scores, static_cast<size_t>(nq) * k, mask,
                   vg::mask_span(mask, nq > 1 ? mask_stride : 0, nq, idx->n)));
    const hipStream_t st = io.st;
    if (idx->n == 0) {
        VG_TRY(vg::empty_results(nq, k, false, io.oid.ptr, io.osc.ptr, st));
    } else {
        const int64_t stride = nq > 1 ? mask_stride : 0;
        VG_TRY(vg::int4_scan_batch(idx, io.q.ptr, nq, k, io.mk.ptr, stride, io.oid.ptr, io.osc.ptr, st));
        // queries whose distances may hold a NaN: the reference's heap, operation by operation (vg_cand_replay.hpp)
        VG_TRY(vg::launch_cand_replay(vg::Int4Scorer{idx->d_int4_rows, idx->int4_table, idx->int4_min, idx->int4_diff, idx->dim}, io.q.ptr,
                                      idx->dim, idx->n, nq, k, false, io.mk.ptr, stride, io.oid.ptr, io.osc.ptr, st));
    }
    return io.finish();
}
