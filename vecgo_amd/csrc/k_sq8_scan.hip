// k_sq8_scan.hip — the SQ8 codes of an index and their search:
//   flat.Segment.Search, SQ8 branch internal/segment/flat/segment.go:517-604
// One GPU lane owns a row (vg_sq8_row.hpp: the quantizer's numerics contract, k_sq8.hip); the scan
// reads codes re-tiled to [tile of 64 rows][16-byte group][lane] (one coalesced 1 KiB request per
// wave-instruction, exactly dim bytes per row when 16 | dim).  q, min and invScale are the same
// for every lane: they are read through wave-uniform (scalar) loads, not per lane.
#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_cand_replay.hpp"
#include "vg_nominate.hpp"
#include "vg_scan_slices.hpp"
#include "vg_search.hpp"
#include "vg_sq8_row.hpp"

namespace vg {

// reference layout -> [tile][group][lane] 16-byte pieces (zero padded past dim and past n)
__global__ void sq8_retile_kernel(const uint8_t *__restrict__ codes, int64_t n, int dim, int groups,
                                  int64_t n_tiles, uint4 *__restrict__ tiles)
{
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t total = n_tiles * groups * 64;
    if (gid >= total) return;
    const int lane = static_cast<int>(gid & 63);
    const int64_t tg = gid >> 6;
    const int g = static_cast<int>(tg % groups);
    const int64_t row = (tg / groups) * 64 + lane;
    uint32_t w[4] = {0, 0, 0, 0};
    if (row < n) {
        const uint8_t *src = codes + row * dim;
        for (int b = 0; b < 16; b++) {
            const int at = g * 16 + b;
            if (at < dim) w[b >> 2] |= static_cast<uint32_t>(src[at]) << (8 * (b & 3));
        }
    }
    tiles[gid] = make_uint4(w[0], w[1], w[2], w[3]);
}

// Exhaustive SQ8 scan with fused top-k.  HBM-bound by design: 16*groups bytes per row.
constexpr int kSqWaves = 4;
constexpr int kSqThreads = kSqWaves * 64;
template <bool DOT, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sq8_scan_kernel(
    const uint4 *__restrict__ tiles, int64_t n_rows, int64_t n_tiles, int groups, int dim,
    const float *__restrict__ queries, const float *__restrict__ mins, const float *__restrict__ inv, int slices,
    int nq, int k, uint64_t *__restrict__ partial, const uint64_t *__restrict__ min_keys)
{
    __shared__ uint64_t lists[WAVES * 64];
    __shared__ int valid[WAVES];
    const int b = blockIdx.x;
    const int xcd = b & 7;
    const int o = b >> 3;
    const int q = o % nq;
    const int s = (o / nq) * 8 + xcd;
    const int64_t t0 = n_tiles * s / slices, t1 = n_tiles * (s + 1) / slices;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *qv = queries + static_cast<int64_t>(q) * dim;
    const int full = dim >> 4, tail = dim & 15;
    WaveTopK tk;
    tk.init(k);
    // one-query passes deal the tiles round-robin over the workgroups (one moving window of the code array, see
    // rabitq_scan_kernel); several queries keep the slice mapping and share the slice in their XCD's L2
    const bool dealt = nq == 1;
    const int64_t step = dealt ? static_cast<int64_t>(slices) * WAVES : WAVES;
    const int64_t end = dealt ? n_tiles : t1;
    int64_t tile = dealt ? static_cast<int64_t>(s) * WAVES + wave : t0 + wave;
    if (tail == 0 && full % kSqAhead == 0 && full >= kSqAhead && tile < end) {  // the ring runs on from tile to tile
        uint4 ring[kSqAhead];
        const uint4 *tp = tiles + (tile * groups) * 64 + lane;
#pragma unroll
        for (int a = 0; a < kSqAhead; a++) ring[a] = load_stream(tp + a * 64);
        for (; tile < end; tile += step) {
            const int64_t tn = tile + step < end ? tile + step : tile;  // (the last tile's own first groups again: unused)
            const uint4 *tpn = tiles + (tn * groups) * 64 + lane;
            const float total = sq8_row_score_stream<DOT>(tp, tpn, full, ring, qv, mins, inv);
            tp = tpn;
            const int64_t row = tile * 64 + lane;
            uint64_t key = row < n_rows ? make_key(total, static_cast<uint32_t>(row), DOT) : kKeyMax;
            if (min_keys && key <= min_keys[q]) key = kKeyMax;  // paged results: only keys after the previous page
            tk.offer(key, lane);
        }
    }
    for (; tile < end; tile += step) {
        const float total = sq8_row_score<DOT>(tiles + (tile * groups) * 64 + lane, groups, full, tail, qv, mins, inv);
        const int64_t row = tile * 64 + lane;
        uint64_t key = row < n_rows ? make_key(total, static_cast<uint32_t>(row), DOT) : kKeyMax;
        if (min_keys && key <= min_keys[q]) key = kKeyMax;  // paged results: only keys after the previous page
        tk.offer(key, lane);
    }
    wg_rank_merge<WAVES>(tk, lists, valid, wave, lane, tid, k,
                          partial + (static_cast<int64_t>(q) * slices + s) * k);
}

// Partition-probed SQ8 scan (flat/segment.go:727-744 over the :517-604 branch): workgroup =
// (slice of one probed partition's tiles, probe, query); rows outside the partition's range are masked.
template <bool DOT, bool MASKED>
__global__ __launch_bounds__(kSqThreads) void sq8_probe_kernel(
    const uint4 *__restrict__ tiles, int64_t n_rows, int groups, int dim, const float *__restrict__ queries,
    const float *__restrict__ mins, const float *__restrict__ inv, const uint32_t *__restrict__ probes,
    const uint32_t *__restrict__ part_off, int np, int sub, int k, uint64_t *__restrict__ partial,
    const uint64_t *__restrict__ min_keys, const uint8_t *__restrict__ mask, int64_t mask_stride)
{
    __shared__ uint64_t lists[kSqWaves * 64];
    __shared__ int valid[kSqWaves];
    const int s = blockIdx.x, j = blockIdx.y;
    const int64_t q = blockIdx.z;
    const uint32_t p = probes[q * np + j];
    const int64_t R0 = part_off[p], R1 = part_off[p + 1];
    const int64_t tt0 = R0 >> 6, tt1 = (R1 + 63) >> 6;
    const int64_t t0 = tt0 + (tt1 - tt0) * s / sub, t1 = tt0 + (tt1 - tt0) * (s + 1) / sub;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *qv = queries + q * dim;
    const uint8_t *mq = MASKED ? mask + q * mask_stride : nullptr;
    const int full = dim >> 4, tail = dim & 15;
    WaveTopK tk;
    tk.init(k);
    for (int64_t tile = t0 + wave; tile < t1; tile += kSqWaves) {
        const int64_t row = tile * 64 + lane;
        // filter.Matches after the batch was scored (segment.go:559-561): the candidates are the rows that pass
        const bool live = row >= R0 && row < R1 && row < n_rows && (!MASKED || mask_bit(mq, row));
        if (MASKED && !__any(live)) continue;  // a tile the filter leaves nothing of: its codes are not read
        const float total = sq8_row_score<DOT>(tiles + (tile * groups) * 64 + lane, groups, full, tail, qv, mins, inv);
        uint64_t key = live ? make_key(total, static_cast<uint32_t>(row), DOT) : kKeyMax;
        if (min_keys && key <= min_keys[q]) key = kKeyMax;  // paged results (k > 64)
        tk.offer(key, lane);
    }
    wg_rank_merge<kSqWaves>(tk, lists, valid, wave, lane, tid, k, partial + ((q * np + j) * sub + s) * k);
}

// The same with the pairs grouped by partition (k_probe.hip): a lane decodes its row's 16 codes of a
// dimension group ONCE and applies them to up to kProbeQB queries held in LDS — the decode (cvt + fma)
// and the code traffic are shared, each query keeps its own 16 lane accumulators (L2) or running sum
// (DotProduct), i.e. exactly the arithmetic of sq8_row_score per (row, query).
constexpr int kSqProbeQ = 4;  // queries per decode pass: 4 x 16 lane accumulators keep two waves per SIMD
template <bool DOT, bool FULL>
__device__ __forceinline__ void sq8_row_scores_mq(const uint4 *__restrict__ tp, int groups, int full, int tail, int cnt,
                                                  const float *qlds, int dimp, const float *__restrict__ mins,
                                                  const float *__restrict__ inv, float (&total)[kSqProbeQ])
{
    float acc[DOT ? 1 : kSqProbeQ][16];
    float run[kSqProbeQ];
#pragma unroll
    for (int qi = 0; qi < kSqProbeQ; qi++) {
        run[qi] = 0.0f;
        if (!DOT) {
#pragma unroll
            for (int l = 0; l < 16; l++) acc[qi][l] = 0.0f;
        }
    }
    uint4 ring[kSqAhead];
    const int glast = groups - 1;
#pragma unroll
    for (int a = 0; a < kSqAhead; a++) ring[a] = tp[(a < glast ? a : glast) * 64];
    const int ngr = full + (tail ? 1 : 0);
    for (int g0 = 0; g0 < ngr; g0 += kSqAhead) {
#pragma unroll
        for (int a = 0; a < kSqAhead; a++) {
            const int g = g0 + a;
            const uint4 c = ring[a];
            const int gn = g + kSqAhead;
            ring[a] = tp[(gn < glast ? gn : glast) * 64];
            if (g >= ngr) continue;
            if (g == full && !DOT) continue;  // the L2 tail is added after the lane tree, below
            const int lim = g < full ? 16 : tail;
            const uint32_t w[4] = {c.x, c.y, c.z, c.w};
            const float *mn = mins + g * 16, *iv = inv + g * 16;
            float rec[16];
#pragma unroll
            for (int l = 0; l < 16; l++) {
                const float cf = static_cast<float>((w[l >> 2] >> (8 * (l & 3))) & 0xFFu);
                if (DOT) {
                    const float t = cf * iv[l < lim ? l : 0];
                    rec[l] = mn[l < lim ? l : 0] + t;
                } else {
                    rec[l] = __builtin_fmaf(cf, iv[l], mn[l]);
                }
            }
#pragma unroll
            for (int qi = 0; qi < kSqProbeQ; qi++) {
                if (FULL || qi < cnt) {
                    const float4 *q4 = reinterpret_cast<const float4 *>(qlds + qi * dimp + g * 16);
                    float qv[16];
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const float4 x = q4[t];
                        qv[4 * t] = x.x; qv[4 * t + 1] = x.y; qv[4 * t + 2] = x.z; qv[4 * t + 3] = x.w;
                    }
                    if (DOT) {
#pragma unroll
                        for (int l = 0; l < 16; l++)
                            if (l < lim) {
                                const float prod = qv[l] * rec[l];
                                run[qi] = run[qi] + prod;
                            }
                    } else {
#pragma unroll
                        for (int l = 0; l < 16; l++) {
                            const float diff = qv[l] - rec[l];
                            acc[qi][l] = __builtin_fmaf(diff, diff, acc[qi][l]);
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < kSqProbeQ; qi++) {
        if (DOT) {
            total[qi] = run[qi];
        } else if (FULL || qi < cnt) {
            float t = reduce16_regs(acc[qi]);
            if (tail) t = sq8_tail(t, tp[full * 64], tail, qlds + qi * dimp + full * 16, mins + full * 16, inv + full * 16);
            total[qi] = t;
        } else {
            total[qi] = 0.0f;
        }
    }
}

// Exhaustive scan of several queries: workgroup = (group of kSqProbeQ queries, slice), every code decoded
// once per group.  Same block order as sq8_scan_kernel: the groups of one slice share an XCD's L2.
template <bool DOT>
__global__ __launch_bounds__(kSqThreads) void sq8_scan_mq_kernel(
    const uint4 *__restrict__ tiles, int64_t n_rows, int64_t n_tiles, int groups, int dim,
    const float *__restrict__ queries, const float *__restrict__ mins, const float *__restrict__ inv, int slices,
    int nq, int k, uint64_t *__restrict__ partial, const uint64_t *__restrict__ min_keys)
{
    extern __shared__ __attribute__((aligned(16))) float qlds[];  // kSqProbeQ * dimp floats, then the merge scratch
    const int dimp = groups * 16;
    uint64_t *lists = reinterpret_cast<uint64_t *>(qlds + static_cast<size_t>(kSqProbeQ) * dimp);
    int *valid = reinterpret_cast<int *>(lists + kSqWaves * 64);
    const int ng = (nq + kSqProbeQ - 1) / kSqProbeQ;
    const int b = blockIdx.x;
    const int xcd = b & 7;
    const int o = b >> 3;
    const int qg = o % ng;
    const int s = (o / ng) * 8 + xcd;
    const int q0 = qg * kSqProbeQ;
    const int cnt = nq - q0 < kSqProbeQ ? nq - q0 : kSqProbeQ;
    const int64_t t0 = n_tiles * s / slices, t1 = n_tiles * (s + 1) / slices;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int qi = 0; qi < cnt; qi++) {
        const float *src = queries + static_cast<int64_t>(q0 + qi) * dim;
        for (int t = tid; t < dimp; t += kSqThreads) qlds[qi * dimp + t] = t < dim ? src[t] : 0.0f;
    }
    __syncthreads();
    const int full = dim >> 4, tail = dim & 15;
    WaveTopK tk[kSqProbeQ];
#pragma unroll
    for (int qi = 0; qi < kSqProbeQ; qi++) tk[qi].init(k);
    for (int64_t tile = t0 + wave; tile < t1; tile += kSqWaves) {
        const uint4 *tp = tiles + (tile * groups) * 64 + lane;
        float total[kSqProbeQ];
        if (cnt == kSqProbeQ)
            sq8_row_scores_mq<DOT, true>(tp, groups, full, tail, cnt, qlds, dimp, mins, inv, total);
        else
            sq8_row_scores_mq<DOT, false>(tp, groups, full, tail, cnt, qlds, dimp, mins, inv, total);
        const int64_t row = tile * 64 + lane;
#pragma unroll
        for (int qi = 0; qi < kSqProbeQ; qi++)
            if (qi < cnt) {
                uint64_t key = row < n_rows ? make_key(total[qi], static_cast<uint32_t>(row), DOT) : kKeyMax;
                if (min_keys && key <= min_keys[q0 + qi]) key = kKeyMax;
                tk[qi].offer(key, lane);
            }
    }
#pragma unroll
    for (int qi = 0; qi < kSqProbeQ; qi++) {
        if (qi < cnt) {
            wg_rank_merge<kSqWaves>(tk[qi], lists, valid, wave, lane, tid, k,
                                    partial + (static_cast<int64_t>(q0 + qi) * slices + s) * k);
            __syncthreads();
        }
    }
}

template <bool DOT>
__global__ __launch_bounds__(kSqThreads) void sq8_probe_mq_kernel(
    const uint4 *__restrict__ tiles, int64_t n_rows, int groups, int dim, const float *__restrict__ queries,
    const float *__restrict__ mins, const float *__restrict__ inv, const uint32_t *__restrict__ part_off,
    const uint32_t *__restrict__ pair_of, const ProbeGroup *__restrict__ pgroups, const uint32_t *__restrict__ ngroups,
    int np, int sub, int k, uint64_t *__restrict__ partial, const uint64_t *__restrict__ min_keys,
    const uint8_t *__restrict__ mask, int64_t mask_stride)
{
    extern __shared__ __attribute__((aligned(16))) float qlds[];  // kProbeQB * dimp floats, then the merge scratch
    const int dimp = groups * 16;
    uint64_t *lists = reinterpret_cast<uint64_t *>(qlds + static_cast<size_t>(kProbeQB) * dimp);
    int *valid = reinterpret_cast<int *>(lists + kSqWaves * 64);
    __shared__ uint32_t pair[kProbeQB];
    if (blockIdx.y >= ngroups[0]) return;
    const ProbeGroup pg = pgroups[blockIdx.y];
    const int s = blockIdx.x, cnt = static_cast<int>(pg.count);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < cnt) pair[tid] = pair_of[pg.first + tid];
    __syncthreads();
    for (int qi = 0; qi < cnt; qi++) {
        const float *src = queries + static_cast<int64_t>(pair[qi] / np) * dim;
        for (int t = tid; t < dimp; t += kSqThreads) qlds[qi * dimp + t] = t < dim ? src[t] : 0.0f;
    }
    __syncthreads();
    const int64_t R0 = part_off[pg.part], R1 = part_off[pg.part + 1];
    const int64_t tt0 = R0 >> 6, tt1 = (R1 + 63) >> 6;
    const int64_t t0 = tt0 + (tt1 - tt0) * s / sub, t1 = tt0 + (tt1 - tt0) * (s + 1) / sub;
    const int full = dim >> 4, tail = dim & 15;
    WaveTopK tk[kProbeQB];
#pragma unroll
    for (int qi = 0; qi < kProbeQB; qi++) tk[qi].init(k);
    for (int64_t tile = t0 + wave; tile < t1; tile += kSqWaves) {
        const uint4 *tp = tiles + (tile * groups) * 64 + lane;
        const int64_t row = tile * 64 + lane;
        const bool live = row >= R0 && row < R1 && row < n_rows;
        if (mask && mask_stride == 0 && !__any(live && mask_bit(mask, row))) continue;  // nothing of the tile passes the filter
        // the group's queries in passes of kSqProbeQ (the second pass finds the tile's codes in L1 / L2)
#pragma unroll
        for (int qb = 0; qb < kProbeQB; qb += kSqProbeQ) {
            if (qb < cnt) {
                float total[kSqProbeQ];
                const int left = cnt - qb;
                if (left >= kSqProbeQ)
                    sq8_row_scores_mq<DOT, true>(tp, groups, full, tail, left, qlds + qb * dimp, dimp, mins, inv, total);
                else
                    sq8_row_scores_mq<DOT, false>(tp, groups, full, tail, left, qlds + qb * dimp, dimp, mins, inv, total);
#pragma unroll
                for (int qi = 0; qi < kSqProbeQ; qi++)
                    if (qb + qi < cnt) {
                        uint64_t key = live ? make_key(total[qi], static_cast<uint32_t>(row), DOT) : kKeyMax;
                        if (min_keys && key <= min_keys[pair[qb + qi] / np]) key = kKeyMax;  // paged results (k > 64)
                        if (mask && live && !mask_bit(mask + static_cast<int64_t>(pair[qb + qi] / np) * mask_stride, row))
                            key = kKeyMax;  // filter.Matches (segment.go:559-561), each query its own mask
                        tk[qb + qi].offer(key, lane);
                    }
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < kProbeQB; qi++) {
        if (qi < cnt) {
            wg_rank_merge<kSqWaves>(tk[qi], lists, valid, wave, lane, tid, k,
                                    partial + (static_cast<int64_t>(pair[qi]) * sub + s) * k);
            __syncthreads();
        }
    }
}

int32_t launch_probe_scan_sq8_grouped(const vg_index *idx, const float *queries, const uint32_t *part_off,
                                      const uint32_t *pair_of, const ProbeGroup *groups, const uint32_t *ngroups, unsigned gmax,
                                      int np, int sub, int k, uint64_t *partial, const uint64_t *min_keys, const uint8_t *mask,
                                      int64_t mask_stride, hipStream_t st)
{
    const bool dot = idx->metric != VG_METRIC_L2;
    auto kern = dot ? sq8_probe_mq_kernel<true> : sq8_probe_mq_kernel<false>;
    const size_t lds = sizeof(float) * kProbeQB * static_cast<size_t>(idx->sq_groups) * 16 + kSqWaves * 64 * sizeof(uint64_t) + 64;
    VG_CHECK(lds <= 152 * 1024, VG_ERR_UNSUPPORTED, "sq8 grouped probe: %d dimensions do not fit LDS", idx->dim);
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(lds)));
    ProfScope prof(idx->ctx, "sq8_probe", st);
    VG_LAUNCH(kern, dim3(static_cast<unsigned>(sub), gmax), dim3(kSqThreads), lds, st,
              reinterpret_cast<const uint4 *>(idx->d_sq_tiles), idx->n, idx->sq_groups, idx->dim, queries, idx->sq->d_mins,
              idx->sq->d_inv, part_off, pair_of, groups, ngroups, np, sub, k, partial, min_keys, mask, mask_stride);
    return VG_OK;
}

int32_t launch_probe_scan_sq8(const vg_index *idx, const float *queries, const uint32_t *probes, const uint32_t *part_off,
                              int64_t nq, int np, int sub, int k, uint64_t *partial, const uint64_t *min_keys,
                              const uint8_t *mask, int64_t mask_stride, hipStream_t st)
{
    for (int64_t q0 = 0; q0 < nq; q0 += 65535) {
        const int64_t cnt = nq - q0 < 65535 ? nq - q0 : 65535;
        ProfScope prof(idx->ctx, "sq8_probe", st);
        auto kern = mask ? (idx->metric != VG_METRIC_L2 ? sq8_probe_kernel<true, true> : sq8_probe_kernel<false, true>)
                         : (idx->metric != VG_METRIC_L2 ? sq8_probe_kernel<true, false> : sq8_probe_kernel<false, false>);
        VG_LAUNCH(kern, dim3(static_cast<unsigned>(sub), static_cast<unsigned>(np), static_cast<unsigned>(cnt)),
                  dim3(kSqThreads), 0, st, reinterpret_cast<const uint4 *>(idx->d_sq_tiles), idx->n, idx->sq_groups, idx->dim,
                  queries + q0 * idx->dim, idx->sq->d_mins, idx->sq->d_inv, probes + q0 * np, part_off, np, sub, k,
                  partial + q0 * np * sub * k, min_keys ? min_keys + q0 : nullptr, mask ? mask + q0 * mask_stride : nullptr,
                  mask_stride);
    }
    return VG_OK;
}

// ---- batched search through a bfloat16 nomination (vg_index_enable_sq8_nomination) ---------------------------------------------
// The multi-query scan decodes every code once per 4 queries and is bound by the vector ALU (44 ms per 1024 queries x 1M x 768).
// With the opt-in image — the dequantised rows x^ = fma(code, invScale, min) rounded to bfloat16, 2 bytes per code — the batch runs
// the shared nomination (vg_nominate.hpp), re-scores with the reference's own arithmetic on the CODES (sq8_row_score, Sq8Row) and
// proves the result (bfloat16 rounding of both operands, fp32 accumulation, the reference's own rounding).  A query whose proof
// fails is scanned as before.
#ifndef VG_SQ8_NOM_MIN_Q
#define VG_SQ8_NOM_MIN_Q 5  // smallest batch the nomination takes: 1M x 768, scan / nominated ms: 4 queries 0.34 / 0.37, 6: 0.51 / 0.38, 16: 0.94 / 0.37
#endif

__device__ __forceinline__ uint16_t sq8_bf16_rne(float x)
{
    const uint32_t b = __float_as_uint(x);
    return static_cast<uint16_t>((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
}

// one lane per row of a 64-row tile: dequantise, round, write the row's bf16 image and its norm
// (rows of dim_pad elements: the dimensions from dim on are zeros, which add nothing to a dot product)
__global__ __launch_bounds__(64) void sq8_dequant_bf16_kernel(const uint4 *__restrict__ tiles, int64_t n, int dim, int groups,
                                                              const float *__restrict__ mins, const float *__restrict__ inv,
                                                              uint16_t *__restrict__ out, int dim_pad, float *__restrict__ norms,
                                                              int *__restrict__ norm_max_bits)
{
    const int64_t tile = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t row = tile * 64 + lane;
    float nrm = 0.0f;
    if (row < n) {
        for (int g = 0; g < dim_pad / 16; g++) {
            const uint4 c = g < groups ? tiles[(tile * groups + g) * 64 + lane] : make_uint4(0, 0, 0, 0);
            const uint32_t w[4] = {c.x, c.y, c.z, c.w};
            uint32_t packed[8];
#pragma unroll
            for (int t = 0; t < 16; t += 2) {
                uint32_t pair = 0;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int j = g * 16 + t + h;
                    float x = 0.0f;
                    if (j < dim) {
                        const float code = static_cast<float>((w[(t + h) >> 2] >> (8 * ((t + h) & 3))) & 0xFFu);
                        x = __builtin_fmaf(code, inv[j], mins[j]);
                    }
                    nrm = __builtin_fmaf(x, x, nrm);
                    pair |= static_cast<uint32_t>(sq8_bf16_rne(x)) << (16 * h);
                }
                packed[t >> 1] = pair;
            }
            uint4 *dst = reinterpret_cast<uint4 *>(out + row * dim_pad + g * 16);
            dst[0] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
            dst[1] = make_uint4(packed[4], packed[5], packed[6], packed[7]);
        }
        norms[row] = nrm;
    }
    // a NaN norm (a NaN in mins / inv) must reach norm_max — fmaxf would drop it, and a finite bound over a row whose GEMM score is
    // NaN would let the proof pass: NaN -> +Inf (the largest bit pattern below), the proof's comparisons then fail and the scan answers
    float mx = row < n ? (nrm == nrm ? nrm : INFINITY) : 0.0f;
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) atomicMax(norm_max_bits, __float_as_int(mx));  // non-negative floats order like their bits
}

// the verify pair's Row (vg_nominate.hpp): exact L2Distance / DotProduct of a nominated row from the codes
template <bool DOT>
struct Sq8Row {
    const uint4 *tiles;
    int groups, dim;
    const float *mins, *inv;
    __device__ float score(int64_t, const float *qv, uint32_t id) const
    {
        return sq8_row_score<DOT>(tiles + (static_cast<int64_t>(id >> 6) * groups) * 64 + (id & 63), groups, dim >> 4, dim & 15, qv, mins, inv);
    }
    // |s~ + |q|^2 - L2Distance|: bfloat16 rounding of q and x^ ((2^-7 + 2^-16)(|q|^2 + |x^|^2), as for the fp32 rows' bf16
    // filter), the GEMM's fp32 accumulation and the reference's own 16-lane sums ((2 dim + dim/8 + 32) u of the same)
    // (Dot: the score is -q.x^, half the L2 form's cross term: 2^-8 in place of 2^-7)
    __device__ float eps(float qn, float norm_max) const
    {
        return (4.0f * (static_cast<float>(dim) * 5.9604645e-8f) + (DOT ? 0.00390625f : 0.0078125f) * 1.02f) * (qn + norm_max) + 1e-30f;
    }
    static constexpr bool kShifted = false;  // (the GEMM multiplies the dequantised rows themselves)
};

// ---- the same from the codes (vg_index_enable_sq8_nomination_from_codes): no image of the dequantised rows -----------------------
// The reference decodes x^_d = float32(c_d) inv_d + min_d (quantizer.go:241-247).  With c'_d = c_d - 128, an integer in -128 .. 127
// that bfloat16 holds exactly, y = c' o inv and mid_d = min_d + 128 inv_d:  q.x^ = (q o inv).c' + q.mid.  The GEMM multiplies the
// query image bf16(q_d inv_d) — the ONLY rounded operand — by the exact c', converted from the code tiles inside the tile's fill
// (flat_gemm_sq8_big_kernel) and, for the sampled tiles, in the call's scratch (sq8_sample_rows_kernel, k_flat.hip): both score
//     s' = |x^|^2 - 2 (q o inv).c'   (Dot: -(q o inv).c'),
// the image mode's space moved by the per-query constant 2 q.mid (Dot: q.mid), which the verify pair takes back (Sq8CodesRow::shift).
// The codes are CENTRED because the query rounding is relative to |q| |c o inv|: uncentred that is |q| |x^ - min|, on normal rows
// about 5 sigma per dimension where |x^ - mid| is about one.
// The state (NomImage, from_codes with `scale`): rows = mid as dim_pad floats (zeros from dim on) and, behind them, one float
// H2 = sum_d (|min_d| + 255 |inv_d|)^2 (Dot's margin); norms = |x^|^2 exactly as the image mode computes them; norm_max =
// max over the rows of max(|x^|^2, |y|^2), so that 2.002 (|q|^2 + norm_max) still lies above every |s'| (flat_thr_cap_kernel:
// |s'| <= |x^|^2 + 2.01 |q||y|) and B = |q|^2 + norm_max scales every term below.  NaN -> +Inf as in the image mode.
__global__ void sq8_mid_kernel(const float *__restrict__ mins, const float *__restrict__ inv, int dim, int dim_pad, float *__restrict__ mid)
{
    float h2 = 0.0f;  // one workgroup of 64 lanes
    for (int j = threadIdx.x; j < dim_pad; j += 64) {
        mid[j] = j < dim ? __builtin_fmaf(128.0f, inv[j], mins[j]) : 0.0f;
        if (j < dim) {
            const float h = fabsf(mins[j]) + 255.0f * fabsf(inv[j]);
            h2 = __builtin_fmaf(h, h, h2);
        }
    }
    for (int off = 32; off > 0; off >>= 1) h2 += __shfl_xor(h2, off);
    if (threadIdx.x == 0) mid[dim_pad] = h2;
}
// one lane per row of a 64-row tile, as sq8_dequant_bf16_kernel without the image: the same |x^|^2, and |y|^2 beside it for norm_max
__global__ __launch_bounds__(64) void sq8_codes_norms_kernel(const uint4 *__restrict__ tiles, int64_t n, int dim, int groups,
                                                             const float *__restrict__ mins, const float *__restrict__ inv,
                                                             float *__restrict__ norms, int *__restrict__ norm_max_bits)
{
    const int64_t tile = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t row = tile * 64 + lane;
    float nrm = 0.0f, cn = 0.0f;
    if (row < n) {
        for (int g = 0; g < groups; g++) {
            const uint4 c = tiles[(tile * groups + g) * 64 + lane];
            const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const int j = g * 16 + t;
                if (j < dim) {
                    const uint32_t code = (w[t >> 2] >> (8 * (t & 3))) & 0xFFu;
                    const float x = __builtin_fmaf(static_cast<float>(code), inv[j], mins[j]);
                    const float y = static_cast<float>(static_cast<int>(code) - 128) * inv[j];
                    nrm = __builtin_fmaf(x, x, nrm);
                    cn = __builtin_fmaf(y, y, cn);
                }
            }
        }
        norms[row] = nrm;
    }
    float mx = 0.0f;
    if (row < n) mx = nrm == nrm && cn == cn ? fmaxf(nrm, cn) : INFINITY;
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) atomicMax(norm_max_bits, __float_as_int(mx));  // non-negative floats order like their bits
}

// the verify pair's Row from the codes: Sq8Row's exact score (the re-score is the same), the score space's constant and its margin
template <bool DOT>
struct Sq8CodesRow : Sq8Row<DOT> {
    const float *mid;  // dim_pad floats, then H2
    int dim_pad;
    static constexpr bool kShifted = true;
    __device__ float shift(const float *qv, int lane) const  // the lane's share of q.mid
    {
        float c = 0.0f;
        for (int j = lane; j < this->dim; j += 64) c = __builtin_fmaf(qv[j], mid[j], c);
        return c;
    }
    // |s' + |q|^2 - 2 q.mid - L2Distance| (Dot: |s' - q.mid - (-DotProduct)|) for any row, in units of B = |q|^2 + norm_max, u = 2^-24:
    //  query rounding   the image is q_d inv_d (1 + d)(1 + b), |d| <= u (the fp32 product), |b| <= 2^-8 (bfloat16, nearest even); the
    //                   products with c' are exact in fp32: |sum - q.y| <= (2^-8 + 2 u) |q||y| <= (2^-9 + u) B; L2 scores twice that
    //  GEMM sum         the tile starts at s (|s| <= 1.501 B for L2, 2.002 B for Dot, by flat_thr_cap_kernel), adds dim products
    //                   (S = sum |products| <= 0.51 B) and the key's fma: screen_gemm_eps's term (k_flat.hip), 4.03 (dim + 16) u
    //                   for L2, 2.52 (dim + 16) u for Dot
    //  norms, x^        L2: the stored |x^|^2 is a sum of dim fmas, dim u B; x^ itself is one fma off c inv + min, u |q||x^| twice: u B
    //  mid, q.mid       mid is one fma (u |mid_d|), the wave's sum dim / 64 fmas and 6 additions: (dim / 64 + 8) u |q||mid|, and
    //                   |mid| <= |x^| + |y| <= 2 sqrt(norm_max), |q||mid| <= B; L2 takes it twice: (dim / 32 + 16) u
    //  the comparison   tau + |q|^2 - 2 q.mid - eps (Dot: -tau + q.mid + eps): three (two) roundings of at most 5 B (3 B), and
    //                   |q|^2 as the kernel sums it, (dim / 64 + 7) u: 16 u + (dim / 64 + 7) u  (Dot: 8 u)
    //  the reference    L2: q - x^ rounded (2 u), 16 lane sums of dim / 16 fmas, the reduction tree and the tail (21): (dim / 16 + 23) u
    //                   |q - x^|^2 <= (dim / 8 + 46) u B.  Dot: a running sum of dim rounded products, (dim + 2) u |q||x^| <=
    //                   (dim / 2 + 1) u B — and its decode rounds c inv BEFORE it adds min: u (|min_d| + 255 |inv_d|) per element, which
    //                   no row's norm bounds (every code of a dimension may be 128): u |q| sqrt(H2) <= u (|q|^2 + H2) / 2
    //  L2:  2^-8 + 2 u + (4.03 (dim + 16) + dim + 1 + dim / 32 + 16 + 16 + dim / 64 + 7 + dim / 8 + 46) u  <=  2^-8 1.001 + (6 dim + 160) u
    //  Dot: 2^-9 + u + (2.52 (dim + 16) + dim / 64 + 8 + 8 + dim / 2 + 1) u  <=  2^-9 1.001 + (3.5 dim + 64) u,  + u (|q|^2 + H2)
    // At dim 768: 4.19e-3 B for L2, beside the image mode's 8.15e-3 (two rounded operands).  Denormal products the matrix unit may
    // flush: below 1e-35 dim, inside the absolute term.  tests/test_sq8_nomination_codes_bound_cpu.py models the sums.
    __device__ float eps(float qn, float norm_max) const
    {
        const float d = static_cast<float>(this->dim), u = 5.9604645e-8f;
        if (DOT) return (0.001953125f * 1.001f + (3.5f * d + 64.0f) * u) * (qn + norm_max) + u * (qn + mid[dim_pad]) + 1e-30f;
        return (0.00390625f * 1.001f + (6.0f * d + 160.0f) * u) * (qn + norm_max) + 1e-30f;
    }
};

// the verify pair over nq query rows whose nomination (thresholds, count, candidates each) the batch search or another file
// produced: the partition-probed scan's (query, probe) pairs (k_probe.hip)
int32_t launch_sq8_verify(vg_index *idx, const float *queries, int64_t nq, const ProbeNominated &nom, int k, uint32_t *ids, float *scores,
                          int *fail, hipStream_t st)
{
    const uint4 *tiles = reinterpret_cast<const uint4 *>(idx->d_sq_tiles);
    if (idx->metric != VG_METRIC_L2)
        return launch_nominated_verify<true>(Sq8Row<true>{tiles, idx->sq_groups, idx->dim, idx->sq->d_mins, idx->sq->d_inv}, queries,
                                             idx->sq_nom.norm_max, nq, nom, k, ids, scores, fail, st);
    return launch_nominated_verify<false>(Sq8Row<false>{tiles, idx->sq_groups, idx->dim, idx->sq->d_mins, idx->sq->d_inv}, queries,
                                          idx->sq_nom.norm_max, nq, nom, k, ids, scores, fail, st);
}
// The nomination from the codes takes more than 128 queries — the persistent tile's batches; the register-staged fill has no
// 128-row form — over the whole segment, unfiltered, from kSq8NomCodesMinPairs (query, row) pairs up (tools/sq8_nominate_codes_time.py;
// test hook VG_SQ8_NOM_CODES_ALWAYS: any number of pairs).
constexpr int64_t kSq8NomCodesMinPairs = 12000000;
// whether a batch takes the nomination (vg_index_enable_sq8_nomination, _from_codes; device queries; mask: the batch's row filter, or null)
bool sq8_nomination_applies(const vg_index *idx, const float *d_queries, int64_t nq, int k, const uint8_t *mask)
{
    const int mode = idx->sq_nom.mode();
    if (mode == 2 && (mask || nq <= 128 || (nq * idx->n < kSq8NomCodesMinPairs && !hook(kHookSq8NomCodesAlways)))) return false;
    return mode && nq >= VG_SQ8_NOM_MIN_Q && k <= kNomMaxK && idx->n > k && aligned16(d_queries);
}
// nominated_pass with the SQ8 re-score (mask: a device row filter per query / for the batch, or null)
int32_t sq8_nominated_pass(vg_index *idx, const float *q, int64_t nq, int k, const uint8_t *mask, int64_t mask_stride, uint32_t *oid,
                           float *osc, hipStream_t st, std::vector<int> &failed)
{
    const bool dot = idx->metric != VG_METRIC_L2, codes = idx->sq_nom.mode() == 2;
    const size_t before = failed.size();
    VG_TRY(nominated_pass(idx, idx->sq_nom, dot, q, nq, k, mask, mask_stride, 0, oid, osc, st, failed,
                          [&](const float *qq, int64_t cnt, const ProbeNominated &nom, float *, uint32_t *ids, float *scores, int *fail) -> int32_t {
                              if (!codes) return launch_sq8_verify(idx, qq, cnt, nom, k, ids, scores, fail, st);
                              const NomImage &img = idx->sq_nom;
                              const uint4 *tiles = reinterpret_cast<const uint4 *>(idx->d_sq_tiles);
                              const float *mid = reinterpret_cast<const float *>(img.rows);
                              if (dot)
                                  return launch_nominated_verify<true>(Sq8CodesRow<true>{{tiles, idx->sq_groups, idx->dim, idx->sq->d_mins, idx->sq->d_inv}, mid, img.dim_pad},
                                                                       qq, img.norm_max, cnt, nom, k, ids, scores, fail, st);
                              return launch_nominated_verify<false>(Sq8CodesRow<false>{{tiles, idx->sq_groups, idx->dim, idx->sq->d_mins, idx->sq->d_inv}, mid, img.dim_pad},
                                                                    qq, img.norm_max, cnt, nom, k, ids, scores, fail, st);
                          }));
    idx->sq_nom_rescanned += static_cast<int64_t>(failed.size() - before);  // (vg_index_sq8_nomination_info)
    return VG_OK;
}

// vg_cand_replay.hpp's scorer for the SQ8 scan: sq.L2Distance / sq.DotProduct of a row's code (flat/segment.go:517-604, :659-667),
// one lane per row of the re-tiled codes.  At risk: a non-finite query value, minimum or inverse scale; magnitudes whose partial
// sums could overflow (|x^_j| <= 255 |inv_j| + |min_j|).
template <bool DOT>
struct Sq8Scorer {
    const uint4 *tiles;
    const float *mins, *inv;
    int groups, dim;
    __device__ bool risk(int64_t, const float *q, int tid) const
    {
        __shared__ int flag;
        __shared__ float bmax;
        if (tid == 0) bmax = 0.0f;
        __syncthreads();
        bool bad = false;
        float b = 0.0f;
        for (int j = tid; j < dim; j += kReplayThreads) {
            const float mn = mins[j], iv = inv[j];
            bad = bad || !is_finite_f32(q[j]) || !is_finite_f32(mn) || !is_finite_f32(iv);
            b = fmaxf(b, 255.0f * fabsf(iv) + fabsf(mn));
        }
        for (int off = 32; off > 0; off >>= 1) b = fmaxf(b, __shfl_xor(b, off));
        if ((tid & 63) == 0) atomicMax(reinterpret_cast<int *>(&bmax), __float_as_int(b));  // non-negative floats order like their bits
        __syncthreads();
        const float bm = bmax;
        for (int j = tid; j < dim; j += kReplayThreads) bad = bad || !(score_bound(fabsf(q[j]), bm, DOT) * static_cast<float>(dim) < 1e38f);
        return block_any(bad, &flag, tid);
    }
    __device__ void prepare(int64_t, const float *, int) const {}
    __device__ void score_chunk(int64_t, const float *q, int64_t row0, int64_t n, int tid, float *out) const
    {
        const int64_t row = row0 + tid;  // (any row: a probed range starts where its partition does, inside a tile of 64)
        if (row >= n) return;
        out[tid] = sq8_row_score<DOT>(tiles + ((row >> 6) * groups) * 64 + (row & 63), groups, dim >> 4, dim & 15, q, mins, inv);
    }
};

// the replay for device buffers: the whole segment, or (probes: nq * np partition ids, part_off) the probed partitions; mask: a
// device row filter per query / for the batch, or null (k_probe.hip calls it for the filtered and the partition-probed scans)
int32_t sq8_nan_replay(vg_index *idx, const float *d_queries, int64_t nq, int k, const uint8_t *d_mask, int64_t mask_stride,
                       const uint32_t *d_probes, int np, const uint32_t *d_part_off, uint32_t *d_ids, float *d_scores, hipStream_t st)
{
    if (idx->n == 0) return VG_OK;
    const uint4 *tiles = reinterpret_cast<const uint4 *>(idx->d_sq_tiles);
    if (idx->metric != VG_METRIC_L2)
        return launch_cand_replay(Sq8Scorer<true>{tiles, idx->sq->d_mins, idx->sq->d_inv, idx->sq_groups, idx->dim}, d_queries, idx->dim, idx->n, nq, k,
                                  true, d_mask, mask_stride, d_ids, d_scores, st, nullptr, d_probes, np, d_part_off);
    return launch_cand_replay(Sq8Scorer<false>{tiles, idx->sq->d_mins, idx->sq->d_inv, idx->sq_groups, idx->dim}, d_queries, idx->dim, idx->n, nq, k,
                              false, d_mask, mask_stride, d_ids, d_scores, st, nullptr, d_probes, np, d_part_off);
}

}  // namespace vg

// vg_index_enable_sq8_nomination (mode 1) and vg_index_enable_sq8_nomination_from_codes (mode 2); fn: the entry point's name.
// As for PQ (k_pq_nominate.hip): turning a mode off, or on again, drops that mode only; turning it on drops the other one too, but
// only once nothing can refuse.
static int32_t sq8_nomination_enable(vg_index *idx, int mode, int32_t on, void *stream, const char *fn)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    if (idx->sq_nom.mode() == mode) VG_TRY(vg::nom_free(idx->sq_nom, st));
    if (!on) return VG_OK;
    VG_CHECK(idx->sq && idx->d_sq_tiles, VG_ERR_NOT_READY, "%s: index has no SQ8 codes", fn);
    VG_TRY(vg::nom_free(idx->sq_nom, st));
    idx->sq_nom_rescanned = 0;
    const uint4 *tiles = reinterpret_cast<const uint4 *>(idx->d_sq_tiles);
    const dim3 grid(static_cast<unsigned>(idx->n_tiles));
    const int dim_pad = vg::nom_dim_pad(idx->dim);
    if (mode == 1)
        return vg::nom_build(idx->sq_nom, idx->n, idx->dim, vg::NomImage::body_bytes(idx->n, dim_pad, false), false, st, [&](const vg::NomImage &b, int *norm_max_bits) {
            hipLaunchKernelGGL(vg::sq8_dequant_bf16_kernel, grid, dim3(64), 0, st, tiles, idx->n, idx->dim, idx->sq_groups, idx->sq->d_mins, idx->sq->d_inv,
                               b.rows, b.dim_pad, b.norms, norm_max_bits);
        });
    // from the codes: mid and H2 in the rows' place (4 dim_pad + 4 bytes), the norms, norm_max
    VG_TRY(vg::nom_build(idx->sq_nom, idx->n, idx->dim, static_cast<int64_t>(dim_pad + 1) * 4, true, st, [&](const vg::NomImage &b, int *norm_max_bits) {
        hipLaunchKernelGGL(vg::sq8_mid_kernel, dim3(1), dim3(64), 0, st, idx->sq->d_mins, idx->sq->d_inv, idx->dim, b.dim_pad, reinterpret_cast<float *>(b.rows));
        hipLaunchKernelGGL(vg::sq8_codes_norms_kernel, grid, dim3(64), 0, st, tiles, idx->n, idx->dim, idx->sq_groups, idx->sq->d_mins, idx->sq->d_inv, b.norms,
                           norm_max_bits);
    }));
    idx->sq_nom.scale = idx->sq->d_inv;  // (the quantizer's: it outlives its codes on the index, vg_index_set_sq8_codes)
    return VG_OK;
}

VG_API int32_t vg_index_enable_sq8_nomination(vg_index *idx, int32_t on, void *stream)
{
    return sq8_nomination_enable(idx, 1, on, stream, "vg_index_enable_sq8_nomination");
}

VG_API int32_t vg_index_enable_sq8_nomination_from_codes(vg_index *idx, int32_t on, void *stream)
{
    return sq8_nomination_enable(idx, 2, on, stream, "vg_index_enable_sq8_nomination_from_codes");
}

VG_API int32_t vg_index_sq8_nomination_info(const vg_index *idx, int32_t *mode, int64_t *held_bytes, int64_t *rescanned)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_index_sq8_nomination_info: NULL index");
    if (mode) *mode = idx->sq_nom.mode();
    if (held_bytes) *held_bytes = idx->sq_nom.held_bytes(idx->n);
    if (rescanned) *rescanned = idx->sq_nom.mode() ? idx->sq_nom_rescanned : 0;
    return VG_OK;
}

VG_API int32_t vg_index_set_sq8_codes(vg_index *idx, vg_sq8 *sq, const uint8_t *codes, void *stream)
{
    VG_CHECK(idx && sq, VG_ERR_INVALID_ARG, "vg_index_set_sq8_codes: NULL index or quantizer");
    VG_CHECK(sq->trained, VG_ERR_NOT_TRAINED, "ScalarQuantizer not trained");
    VG_CHECK(sq->dim == idx->dim, VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
    VG_CHECK(idx->n == 0 || codes, VG_ERR_INVALID_ARG, "vg_index_set_sq8_codes: codes is NULL");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    if (idx->d_sq_tiles) {
        VG_HIP(hipStreamSynchronize(st));
        VG_HIP(hipFree(idx->d_sq_tiles));
        idx->d_sq_tiles = nullptr;
    }
    VG_TRY(vg::nom_free(idx->sq_nom, st));  // the old codes' nomination (vg_index_enable_sq8_nomination / _from_codes again after new codes)
    idx->sq = sq;
    idx->sq_groups = (idx->dim + 15) / 16;
    idx->n_tiles = (idx->n + 63) / 64;
    if (idx->n == 0) return VG_OK;
    const int64_t total = idx->n_tiles * idx->sq_groups * 64;
    VG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_sq_tiles), static_cast<size_t>(total) * 16));
    vg::DevIn<uint8_t> in;
    VG_TRY(in.init(codes, static_cast<size_t>(idx->n) * idx->dim, st));
    VG_LAUNCH(vg::sq8_retile_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st, in.ptr, idx->n,
              idx->dim, idx->sq_groups, idx->n_tiles, reinterpret_cast<uint4 *>(idx->d_sq_tiles));
    VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}

static int32_t sq8_search_impl(vg_index *idx, const float *queries, int64_t nq, int32_t k, uint32_t *ids, float *scores, void *stream,
                               bool allow_nomination)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_search_sq8: NULL index");
    VG_CHECK(nq >= 0 && k >= 0, VG_ERR_INVALID_ARG, "vg_search_sq8: negative nq or k");
    if (nq == 0 || k == 0) return VG_OK;
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: Hamming");
    const bool dot = idx->metric != VG_METRIC_L2;  // segment.go:659-667: sq.L2Distance or sq.DotProduct
    VG_CHECK(idx->n == 0 || idx->d_sq_tiles, VG_ERR_NOT_READY, "vg_search_sq8: index has no SQ8 codes");
    VG_CHECK(queries && ids && scores, VG_ERR_INVALID_ARG, "vg_search_sq8: NULL buffer");
    VG_CHECK(k <= 512, VG_ERR_UNSUPPORTED, "vg_search_sq8: k=%d exceeds 512", k);
    vg::SearchIO io;
    VG_TRY(io.init(idx->ctx, stream, queries, static_cast<size_t>(nq) * idx->dim, ids, scores, static_cast<size_t>(nq) * k));
    const hipStream_t st = io.st;
    const float *q = io.q.ptr;
    uint32_t *oid = io.oid.ptr;
    float *osc = io.osc.ptr;
    if (idx->n == 0) {
        VG_TRY(vg::empty_results(nq, k, false, oid, osc, st));
    } else if (allow_nomination && vg::sq8_nomination_applies(idx, q, nq, k, nullptr)) {
        std::vector<int> failed;
        VG_TRY(vg::sq8_nominated_pass(idx, q, nq, k, nullptr, 0, oid, osc, st, failed));
        // the scan kernels for the queries whose proof failed (ties at the k-th score, thresholds too tight)
        VG_TRY(vg::rescan_failed(failed, q, idx->dim, k, nullptr, 0, 0, oid, osc, st,
                                 [&](const float *fq, int64_t nf, const uint8_t *, int64_t, uint32_t *fid, float *fsc) {
                                     return sq8_search_impl(idx, fq, nf, k, fid, fsc, st, false);
                                 }));
    } else {
        // two or more queries: groups of kSqProbeQ share every decode (sq8_scan_mq_kernel)
        const size_t mq_lds = sizeof(float) * vg::kSqProbeQ * static_cast<size_t>(idx->sq_groups) * 16 +
                              vg::kSqWaves * 64 * sizeof(uint64_t) + 64;
        const bool mq = nq >= 2 && mq_lds <= 128 * 1024;
        const int64_t units = mq ? (nq + vg::kSqProbeQ - 1) / vg::kSqProbeQ : nq;  // workgroups per slice
        const int slices = vg::scan_slices(units, idx->n_tiles, idx->ctx->compute_units, 4);  // ~4 workgroups per CU
        vg::ArenaCall ar(idx->ctx, st);
        vg::PagedTopK pages;
        pages.add(ar, nq, k, slices);
        VG_TRY(ar.commit());
        auto mq_kern = dot ? vg::sq8_scan_mq_kernel<true> : vg::sq8_scan_mq_kernel<false>;
        if (mq)
            VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(mq_kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(mq_lds)));
        VG_TRY(pages.run(ar, slices, dot, oid, osc, st, [&](int kk, uint64_t *partial, const uint64_t *floor) -> int32_t {
            if (mq) {
                const int64_t max_q = ((1ll << 30) / slices) * vg::kSqProbeQ;  // whole groups per launch
                for (int64_t q0 = 0; q0 < nq; q0 += max_q) {
                    const int64_t cnt = nq - q0 < max_q ? nq - q0 : max_q;
                    const int64_t ng = (cnt + vg::kSqProbeQ - 1) / vg::kSqProbeQ;
                    vg::ProfScope prof(idx->ctx, "sq8_scan", st);
                    VG_LAUNCH(mq_kern, dim3(static_cast<unsigned>(ng * slices)), dim3(vg::kSqThreads), mq_lds, st,
                              reinterpret_cast<const uint4 *>(idx->d_sq_tiles), idx->n, idx->n_tiles, idx->sq_groups, idx->dim,
                              q + q0 * idx->dim, idx->sq->d_mins, idx->sq->d_inv, slices, static_cast<int>(cnt), kk,
                              partial + q0 * slices * kk, floor ? floor + q0 : nullptr);
                }
            } else {
                const int64_t max_q = (1ll << 30) / slices;
                for (int64_t q0 = 0; q0 < nq; q0 += max_q) {
                    const int64_t cnt = nq - q0 < max_q ? nq - q0 : max_q;
                    vg::ProfScope prof(idx->ctx, "sq8_scan", st);
                    // one query: workgroups of 8 waves (32 waves per CU).  The row loop keeps fewer bytes in flight than
                    // its load ring suggests (the compiler drains it at every group), so the single pass wants the
                    // occupancy: 4M x 768 scan kernel 540 -> 518 us, call 590 -> 559 us (8 workgroups of 4 waves: 500 us,
                    // but the merge of twice the lists gives it back)
                    const bool wide = nq == 1 && idx->n_tiles >= static_cast<int64_t>(slices) * 8;
                    auto kern = wide ? (dot ? vg::sq8_scan_kernel<true, 8> : vg::sq8_scan_kernel<false, 8>)
                                     : (dot ? vg::sq8_scan_kernel<true, vg::kSqWaves> : vg::sq8_scan_kernel<false, vg::kSqWaves>);
                    VG_LAUNCH(kern, dim3(static_cast<unsigned>(cnt * slices)), dim3(wide ? 512 : vg::kSqThreads), 0, st,
                              reinterpret_cast<const uint4 *>(idx->d_sq_tiles), idx->n, idx->n_tiles, idx->sq_groups, idx->dim,
                              q + q0 * idx->dim, idx->sq->d_mins, idx->sq->d_inv, slices, static_cast<int>(cnt), kk,
                              partial + q0 * slices * kk, floor ? floor + q0 : nullptr);
                }
            }
            return VG_OK;
        }));
    }
    // queries whose scores may hold a NaN: the reference's heap, operation by operation (vg_cand_replay.hpp; not for the
    // queries this function sends to itself after a failed proof: the caller's pass covers them)
    if (idx->n > 0 && allow_nomination) VG_TRY(vg::sq8_nan_replay(idx, q, nq, k, nullptr, 0, nullptr, 0, nullptr, oid, osc, st));
    return io.finish();
}

VG_API int32_t vg_search_sq8(vg_index *idx, const float *queries, int64_t nq, int32_t k, uint32_t *ids,
                             float *scores, void *stream)
{
    return sq8_search_impl(idx, queries, nq, k, ids, scores, stream, true);
}
