// vg_node_score.hpp — how one wavefront of a graph walk scores the <= 64 neighbours of a popped node, one id per lane:
//   F32ScorerT, PqScorerT      the HNSW walks' scorers (k_graph.hip, k_hnsw_build.hip, ...) with the PQ arithmetic under them,
//                              which the PQ table builder and the PQ trainer use too (k_pq.hip, k_pq_train.hip)
//   VamanaScorer<kind>::type   the six node scorers of the DiskANN walk (vamana_search_kernel, k_graph.hip)
#pragma once

#include <type_traits>

#include "vg_cand_replay.hpp"
#include "vg_device.hpp"
#include "vg_exact.hpp"
#include "../../include/vecgo_hip.h"
#include "vg_heap.hpp"

namespace vg {

// the gather of fp32 rows, 16 lanes per row and 4 rows at a time: f(mine, id) runs on the 16 lanes that share the row of
// node `id`, held by lane `mine` of `mask`, until every lane of `mask` has had its turn
template <class F>
__device__ __forceinline__ void for_rows16(uint64_t mask, uint32_t id_lane, int lane, F f)
{
    while (mask) {
        const int mine = take4(mask, lane);
        const uint32_t id = __shfl(id_lane, mine < 0 ? 0 : mine);
        if (mine >= 0) f(mine, id);
    }
}

// distance of one node as hnsw wraps it (vectorstore/columnar.go:37-44), all lanes of the 16-lane group
template <bool QLDS = false>
__device__ __forceinline__ float hnsw_node_dist(const float *__restrict__ base, int dim, int metric,
                                                const float *__restrict__ qv, uint32_t id, Sub16 sub)
{
    const float *row = base + static_cast<int64_t>(id) * dim;
    if (metric == kMetricDot) return -exact_pair16<true, kPair, false, QLDS>(row, qv, dim, sub);
    const float d = exact_pair16<false, kPair, false, QLDS>(row, qv, dim, sub);
    return metric == kMetricCos ? 0.5f * d : d;
}

// ---- node scorers ------------------------------------------------------------------------------------
// A scorer fills nb_pair[j] (what distFunc returns) and nb_bnd[j] (what SquaredL2Bounded run to completion
// returns) for every lane j set in `mask`, lane j holding node id_lane.
template <bool QLDS>
struct F32ScorerT {  // fp32 rows: 16 lanes per row, 4 rows at a time, reference summation order; QLDS: qv points into LDS
    const float *base;
    const float *qv;
    int dim, metric;
    Sub16 sub;
    static constexpr bool kBounded = true;  // SquaredL2Bounded exists for the L2 metric (hnsw.go:1353-1366)
    __device__ __forceinline__ static void sync() { __syncthreads(); }  // one wave per workgroup
    __device__ __forceinline__ float one(uint32_t id) const { return hnsw_node_dist<QLDS>(base, dim, metric, qv, id, sub); }
    __device__ __forceinline__ void many(uint64_t mask, uint32_t id_lane, int lane, float *nb_pair, float *nb_bnd) const
    {
        for_rows16(mask, id_lane, lane, [&](int mine, uint32_t id) {
            const float *row = base + static_cast<int64_t>(id) * dim;
            float dp, db;
            if (metric == kMetricDot) {
                dp = -exact_pair16<true, kPair, false, QLDS>(row, qv, dim, sub);
                db = dp;
            } else {
                exact_l2_both16<false, QLDS>(row, qv, dim, sub, dp, db);
                if (metric == kMetricCos) dp = 0.5f * dp;
            }
            if ((lane & 15) == 0) {
                nb_pair[mine] = dp;
                nb_bnd[mine] = db;
            }
        });
    }
};

// ComputeAsymmetricDistance's sum over NG groups of 16 sub-quantizers starting at s0: the NG 16-byte code loads are
// issued together, then the 16*NG table reads (their addresses depend on the code bytes) together — two dependent
// round trips for the whole chunk — and the terms are added in sub-quantizer order, as the reference adds them.
template <int NG>
__device__ __forceinline__ float pq_asym_chunk(const uint8_t *__restrict__ code, const float *__restrict__ lut, int s0,
                                               float distance)
{
    uint4 c[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) c[g] = *reinterpret_cast<const uint4 *>(code + s0 + 16 * g);
    float t[NG * 16];
#pragma unroll
    for (int g = 0; g < NG; g++) {
        const uint32_t w[4] = {c[g].x, c[g].y, c[g].z, c[g].w};
#pragma unroll
        for (int u = 0; u < 16; u++) t[g * 16 + u] = lut[(s0 + g * 16 + u) * 256 + ((w[u >> 2] >> (8 * (u & 3))) & 0xFFu)];
    }
#pragma unroll
    for (int i = 0; i < NG * 16; i++) distance = distance + t[i];
    return distance;
}

// pq.ComputeAsymmetricDistance (pq.go:234-260) of one node's code from the query's table (m * 256 floats in HBM/L2):
// term(s) = the BuildDistanceTable entry of code byte s, summed sequentially over the sub-quantizers.
__device__ __forceinline__ float pq_asym_distance(const uint8_t *__restrict__ code, const float *__restrict__ lut, int m)
{
    float distance = 0.0f;
    int s0 = 0;
    if ((m & 15) == 0) {  // rows of 16-byte multiples are 16-byte aligned (the code array is)
        for (; s0 + 96 <= m; s0 += 96) distance = pq_asym_chunk<6>(code, lut, s0, distance);
        for (; s0 + 32 <= m; s0 += 32) distance = pq_asym_chunk<2>(code, lut, s0, distance);
        for (; s0 + 16 <= m; s0 += 16) distance = pq_asym_chunk<1>(code, lut, s0, distance);
    }
    for (int s = s0; s < m; s++) distance = distance + lut[s * 256 + code[s]];
    return distance;
}

using F32Scorer = F32ScorerT<false>;

// ---- ComputeAsymmetricDistance without a table (sub-dimension 8) ------------------------------------------------
// term(s) = squaredL2Int8DequantizedGeneric (kernels.go:354-362) of the node's centroid of sub-quantizer s: per
// dimension  v = float32(int8)*scale ; v = v + offset ; d = q - v ; dd = d*d ; sum = sum + dd  — five separately
// rounded fp32 operations, summed in order: bit for bit the BuildDistanceTable entry of that centroid
// (pq.go:468-491), computed from the quantizer's own int8 codebook (m * 256 * 8 bytes, shared by every query: L2 /
// L1 hits) instead of being looked up in a per-query table.
// One node per lane, TWO sub-quantizers at a time: every operation of the pair (s, s+1) is one packed-fp32
// instruction on the register pair (term s, term s+1) — v_pk_mul_f32 / v_pk_add_f32 round each half exactly like
// the scalar instruction — so a term costs 8 conversions + 20 half-instructions instead of 48.  The pair's constants
// (its 2 x 8 query floats interleaved, the two scales, the two offsets: 20 floats) are laid out once per query in
// the wave's LDS (pq_direct_prepare) and arrive by broadcast reads: no scalar-load round trip per term (the first
// version waited ~96 of them per call), no vector instruction spent on constants.
typedef float vg_f2 __attribute__((ext_vector_type(2)));
constexpr int kPqPairFloats = 20;  // per pair of sub-quantizers: q interleaved [16], scales [2], offsets [2]

// the wave lays out its query's constants: qprep[(s/2)*20 + ...]; m even
__device__ __forceinline__ void pq_direct_prepare(float *qprep, const float *__restrict__ qv,
                                                  const float *__restrict__ scales, const float *__restrict__ offsets,
                                                  int m, int lane)
{
    for (int e = lane; e < (m >> 1) * kPqPairFloats; e += 64) {
        const int p = e / kPqPairFloats, r = e - p * kPqPairFloats;
        float v;
        if (r < 16)
            v = qv[(2 * p + (r & 1)) * 8 + (r >> 1)];
        else if (r < 18)
            v = scales[2 * p + (r - 16)];
        else
            v = offsets[2 * p + (r - 18)];
        qprep[e] = v;
    }
}

// terms of sub-quantizers (s, s+1): centroids ea / eb, constants at `pc` (LDS); returns (term s, term s+1)
__device__ __forceinline__ vg_f2 pq_term8_pair(uint2 ea, uint2 eb, const float *pc)
{
    const float4 *c4 = reinterpret_cast<const float4 *>(pc);
    const float4 k0 = c4[0], k1 = c4[1], k2 = c4[2], k3 = c4[3], k4 = c4[4];
    const vg_f2 q[8] = {{k0.x, k0.y}, {k0.z, k0.w}, {k1.x, k1.y}, {k1.z, k1.w},
                        {k2.x, k2.y}, {k2.z, k2.w}, {k3.x, k3.y}, {k3.z, k3.w}};
    const vg_f2 scale = {k4.x, k4.y}, offset = {k4.z, k4.w};
    vg_f2 sum = {0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t wa = j < 4 ? ea.x : ea.y, wb = j < 4 ? eb.x : eb.y;
        const vg_f2 f = {static_cast<float>(static_cast<int>(static_cast<int8_t>(wa >> (8 * (j & 3))))),
                         static_cast<float>(static_cast<int>(static_cast<int8_t>(wb >> (8 * (j & 3)))))};
        vg_f2 v = f * scale;
        v = v + offset;
        const vg_f2 d = q[j] - v;
        const vg_f2 dd = d * d;
        sum = sum + dd;
    }
    return sum;
}

// FOUR sub-quantizers (s .. s+3) as two packed pairs whose dependent chains are interleaved statement by statement: a
// packed-fp32 result cannot feed the next instruction (the compiler pads every link of a lone chain with an s_nop:
// 0.7 per v_pk op in the r03 walk), so a lane that carries one chain issues at half rate; two chains fill each other's
// gaps.  Every operation and its operands are pq_term8_pair's: (term s, term s+1) -> a, (term s+2, term s+3) -> b.
__device__ __forceinline__ void pq_term8_quad(uint2 e0, uint2 e1, uint2 e2, uint2 e3, const float *pc, vg_f2 &a, vg_f2 &b)
{
    const float4 *c4 = reinterpret_cast<const float4 *>(pc);
    const float4 k0 = c4[0], k1 = c4[1], k2 = c4[2], k3 = c4[3], k4 = c4[4];
    const float4 m0 = c4[5], m1 = c4[6], m2 = c4[7], m3 = c4[8], m4 = c4[9];  // the next pair's constants: + kPqPairFloats floats
    const vg_f2 qa[8] = {{k0.x, k0.y}, {k0.z, k0.w}, {k1.x, k1.y}, {k1.z, k1.w},
                         {k2.x, k2.y}, {k2.z, k2.w}, {k3.x, k3.y}, {k3.z, k3.w}};
    const vg_f2 qb[8] = {{m0.x, m0.y}, {m0.z, m0.w}, {m1.x, m1.y}, {m1.z, m1.w},
                         {m2.x, m2.y}, {m2.z, m2.w}, {m3.x, m3.y}, {m3.z, m3.w}};
    const vg_f2 sa = {k4.x, k4.y}, oa = {k4.z, k4.w}, sb = {m4.x, m4.y}, ob = {m4.z, m4.w};
    vg_f2 suma = {0.0f, 0.0f}, sumb = {0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int sh = 8 * (j & 3);
        const uint32_t w0 = j < 4 ? e0.x : e0.y, w1 = j < 4 ? e1.x : e1.y, w2 = j < 4 ? e2.x : e2.y, w3 = j < 4 ? e3.x : e3.y;
        const vg_f2 fa = {static_cast<float>(static_cast<int>(static_cast<int8_t>(w0 >> sh))),
                          static_cast<float>(static_cast<int>(static_cast<int8_t>(w1 >> sh)))};
        const vg_f2 fb = {static_cast<float>(static_cast<int>(static_cast<int8_t>(w2 >> sh))),
                          static_cast<float>(static_cast<int>(static_cast<int8_t>(w3 >> sh)))};
        vg_f2 va = fa * sa;
        vg_f2 vb = fb * sb;
        va = va + oa;
        vb = vb + ob;
        const vg_f2 da = qa[j] - va;
        const vg_f2 db = qb[j] - vb;
        const vg_f2 dda = da * da;
        const vg_f2 ddb = db * db;
        suma = suma + dda;
        sumb = sumb + ddb;
    }
    a = suma;
    b = sumb;
}

// scalar form (an odd last sub-quantizer; constants from global memory)
__device__ __forceinline__ float pq_term8(uint2 e, const float *__restrict__ q, float scale, float offset)
{
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t w = j < 4 ? e.x : e.y;
        float v = static_cast<float>(static_cast<int>(static_cast<int8_t>(w >> (8 * (j & 3))))) * scale;
        v = v + offset;
        const float d = q[j] - v;
        const float dd = d * d;
        sum = sum + dd;
    }
    return sum;
}

#ifndef VG_PQ_DIRECT_NG
#define VG_PQ_DIRECT_NG 2  // groups of 16 centroid loads in flight per lane (32 registers per group)
#endif
// NG groups of 16 sub-quantizers from s0: the NG code loads, then the 16 * NG centroid loads, are issued together;
// the terms are added in sub-quantizer order
template <int NG>
__device__ __forceinline__ float pq_direct_chunk(const uint8_t *__restrict__ code, const uint2 *__restrict__ cb,
                                                 const float *qprep, int s0, float distance)
{
    uint4 c[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) c[g] = *reinterpret_cast<const uint4 *>(code + s0 + 16 * g);
    uint2 e[NG * 16];
#pragma unroll
    for (int g = 0; g < NG; g++) {
        const uint32_t w[4] = {c[g].x, c[g].y, c[g].z, c[g].w};
#pragma unroll
        for (int u = 0; u < 16; u++) e[g * 16 + u] = cb[(s0 + g * 16 + u) * 256 + ((w[u >> 2] >> (8 * (u & 3))) & 0xFFu)];
    }
#if defined(VG_PQ_LOAD_PROBE) && VG_PQ_LOAD_PROBE == 1  // stage probe (tools/build_variant.sh): every centroid gather twice
#pragma unroll
    for (int g = 0; g < NG; g++) {
        const uint32_t w[4] = {c[g].x, c[g].y, c[g].z, c[g].w};
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const uint2 x = cb[(s0 + g * 16 + u) * 256 + (((w[u >> 2] >> (8 * (u & 3))) & 0xFFu) ^ 0x55u)];
            asm volatile("" ::"v"(x.x), "v"(x.y));
        }
    }
#endif
#pragma unroll
    for (int i = 0; i < NG * 16; i += 4) {  // s0 is a multiple of 16: whole quads, pairs (s0 + i) / 2 and the next one
        vg_f2 ta, tb;
#if defined(VG_PQ_LOAD_PROBE) && VG_PQ_LOAD_PROBE == 2  // stage probe: every term's arithmetic twice
        {
            uint2 a0 = e[i], a1 = e[i + 1], a2 = e[i + 2], a3 = e[i + 3];
            asm volatile("" : "+v"(a0.x), "+v"(a1.x), "+v"(a2.x), "+v"(a3.x));
            vg_f2 ua, ub;
            pq_term8_quad(a0, a1, a2, a3, qprep + ((s0 + i) >> 1) * kPqPairFloats, ua, ub);
            asm volatile("" ::"v"(ua.x), "v"(ua.y), "v"(ub.x), "v"(ub.y));
        }
#endif
        pq_term8_quad(e[i], e[i + 1], e[i + 2], e[i + 3], qprep + ((s0 + i) >> 1) * kPqPairFloats, ta, tb);
        distance = distance + ta.x;  // the terms join the sum in sub-quantizer order (pq.go:242-257)
        distance = distance + ta.y;
        distance = distance + tb.x;
        distance = distance + tb.y;
    }
    return distance;
}

__device__ __forceinline__ float pq_direct_distance(const uint8_t *__restrict__ code, const int8_t *__restrict__ codebooks,
                                                    const float *__restrict__ scales, const float *__restrict__ offsets,
                                                    const float *__restrict__ qv, const float *qprep, int m)
{
    const uint2 *cb = reinterpret_cast<const uint2 *>(codebooks);
    float distance = 0.0f;
    int s0 = 0;
    if ((m & 15) == 0) {  // rows of 16-byte multiples are 16-byte aligned (the code array is)
        for (; s0 + 16 * VG_PQ_DIRECT_NG <= m; s0 += 16 * VG_PQ_DIRECT_NG)
            distance = pq_direct_chunk<VG_PQ_DIRECT_NG>(code, cb, qprep, s0, distance);
        for (; s0 + 16 <= m; s0 += 16) distance = pq_direct_chunk<1>(code, cb, qprep, s0, distance);
    }
    for (; s0 + 2 <= m; s0 += 2) {
        const vg_f2 t = pq_term8_pair(cb[s0 * 256 + code[s0]], cb[(s0 + 1) * 256 + code[s0 + 1]],
                                      qprep + (s0 >> 1) * kPqPairFloats);
        distance = distance + t.x;
        distance = distance + t.y;
    }
    if (s0 < m) distance = distance + pq_term8(cb[s0 * 256 + code[s0]], qv + s0 * 8, scales[s0], offsets[s0]);
    return distance;
}

// The DiskANN walk's STRICT pass asks a scorer's risk() whether a distance of this query may be a NaN or an Inf: the test of
// vg_cand_replay.hpp's scorers (FlatF32Scorer::risk and the code scorers' beside their scans) on a walk's inputs — a non-finite
// query value or index datum, or magnitudes whose partial sums could overflow.  `bad`, `vm`: what this lane saw of the index's
// data, and the largest |value| of a row among them; true in any lane = at risk.
__device__ __forceinline__ bool walk_risk(const float *qv, int dim, bool bad, float vm, bool as_dot, int lane)
{
    for (int j = lane; j < dim; j += 64) bad = bad || !is_finite_f32(qv[j]);
    for (int off = 32; off > 0; off >>= 1) vm = fmaxf(vm, __shfl_xor(vm, off));
    bad = bad || !is_finite_f32(vm);
    for (int j = lane; j < dim; j += 64) bad = bad || !(score_bound(fabsf(qv[j]), vm, as_dot) * static_cast<float>(dim) < 1e38f);
    return bad;
}

// PQ codes: pq.ComputeAsymmetricDistance (pq.go:234-260) — the way the reference scores graph nodes from PQ
// codes (diskann/segment.go:536-557): term(s) = squaredL2Int8Dequantized of the node's centroid, summed
// sequentially over the sub-quantizers.  One node per lane.
// r02 read every term from the query's BuildDistanceTable image (m * 256 floats = 96 KiB) in global memory: a popped
// node's ~58 fresh neighbours look up random centroids of every sub-quantizer, so one pop pulls nearly the whole
// table through L1, and thousands of resident queries' tables (805 MB for 8192 queries) live in neither L2 nor the
// 256 MB memory-side cache — the walk ran at the HBM rate of its TABLE traffic (18.9 GB per launch against 0.93 GB
// of codes, profiles/r02_traffic.json).  `cb` != nullptr (sub-dimension 8): the terms are computed from the shared
// codebook instead, as the reference computes them; nothing per query is built or kept in memory.
// DIRECT: one kernel instance per form (the table form's loads beside the direct form's set a higher register budget)
template <bool DIRECT>
struct PqScorerT {
    const uint8_t *rows;  // n * m code bytes
    const float *lut;     // m * 256 (table form: sub-dimensions other than 8)
    const int8_t *cb;     // m * 256 * 8 int8 (direct form) or nullptr
    const float *scales, *offsets, *qv;
    float *qprep;         // LDS: pq_direct_prepare's image of this query (direct form), lds_bytes(m) of it
    int m;
    int dim = 0;          // risk() only
    static constexpr bool kBounded = false;
    __host__ __device__ static constexpr size_t lds_bytes(int m, int /*rq_nb*/ = 0) { return DIRECT ? (m >> 1) * kPqPairFloats * sizeof(float) : 0; }
    __device__ __forceinline__ void prepare(int lane) const
    {
        if constexpr (DIRECT) {
            pq_direct_prepare(qprep, qv, scales, offsets, m, lane);
            __syncthreads();
        }
    }
    __device__ __forceinline__ bool risk(int lane) const  // (see walk_risk)
    {
        bool bad = false;
        float vm = 0.0f;
        for (int j = lane; j < m; j += 64) {
            bad = bad || !is_finite_f32(scales[j]) || !is_finite_f32(offsets[j]);
            vm = fmaxf(vm, 128.0f * fabsf(scales[j]) + fabsf(offsets[j]));
        }
        return walk_risk(qv, dim, bad, vm, false, lane);
    }
    __device__ __forceinline__ static void sync() { __syncthreads(); }
    __device__ __forceinline__ float lane_score(uint32_t id) const
    {
#if defined(VG_PQ_PROBE) && VG_PQ_PROBE == 2  // stage probe (tools/build_variant.sh): no scoring work at all
        return __uint_as_float(0x40000000u | (((id * 2654435761u) ^ static_cast<uint32_t>(reinterpret_cast<uintptr_t>(qv) >> 4)) >> 9));
#endif
        const uint8_t *code = rows + static_cast<int64_t>(id) * m;
        if constexpr (DIRECT)
            return pq_direct_distance(code, cb, scales, offsets, qv, qprep, m);
        else
            return pq_asym_distance(code, lut, m);
    }
    __device__ __forceinline__ float one(uint32_t id) const { return lane_score(id); }
    __device__ __forceinline__ void many(uint64_t mask, uint32_t id_lane, int lane, float *nb_pair, float *nb_bnd) const
    {
        if ((mask >> lane) & 1) {
            const float d = lane_score(id_lane);
            nb_pair[lane] = d;
            nb_bnd[lane] = d;
        }
    }
    __device__ __forceinline__ void many(uint64_t mask, uint32_t id_lane, int lane, float *out) const
    {
        if ((mask >> lane) & 1) out[lane] = lane_score(id_lane);
    }
};

// ---- the DiskANN walk's node scorers (searchInternal's distFunc, diskann/segment.go:512-565) ----------------------------------
// VamanaScorer<kind>::type, an aggregate of the arguments of vamana_search_kernel it reads, offers
//   prepare(lane)                    the scorer's LDS staging, ending in the barrier it needs
//   many(mask, id_lane, lane, out)   out[j] = distFunc(query, node of lane j) for every lane j of `mask` (no barrier)
//   risk(lane)                       the STRICT pass's test of the inputs (walk_risk above; RaBitQ has its own); true in any lane:
//                                    the query is walked again with the reference's CandidateHeap
//   lds_bytes(pq_m, rq_nb)           dynamic LDS the scorer stages into: the launch's size, and the offset of what follows it
enum { kVamanaF32 = 0, kVamanaPQ = 1, kVamanaRaBitQ = 2, kVamanaInt4 = 3, kVamanaPQDirect = 4, kVamanaInt4Direct = 5 /* 4, 5: kernel instances only */ };

struct VamanaF32Scorer {  // distance.Provider(metric): SquaredL2 or Dot as they are, 16 lanes per row
    const float *base, *qv, *absmax;
    int dim;
    bool dot;
    Sub16 sub;
    __host__ __device__ static constexpr size_t lds_bytes(int, int) { return 0; }
    __device__ __forceinline__ void prepare(int) const {}
    __device__ __forceinline__ void many(uint64_t mask, uint32_t id_lane, int lane, float *out) const
    {
        for_rows16(mask, id_lane, lane, [&](int mine, uint32_t id) {
            const float *row = base + static_cast<int64_t>(id) * dim;
            const float d = dot ? exact_pair16<true, kPair>(row, qv, dim, sub) : exact_pair16<false, kPair>(row, qv, dim, sub);
            if ((lane & 15) == 0) out[mine] = d;
        });
    }
    __device__ __forceinline__ bool risk(int lane) const { return walk_risk(qv, dim, false, absmax[0], dot, lane); }
};

template <bool DIRECT>
struct VamanaInt4Scorer {  // iq.L2Distance (diskann/segment.go:558-565) = int4L2DistancePrecomputedAvx512 order, one node per lane
    const float *qv, *table, *mn, *diff;  // DIRECT: the table's terms evaluated in place (int4_l2_direct, vg_device.hpp)
    const uint8_t *rows;
    vg_f2v *pairs;
    int dim;
    __host__ __device__ static constexpr size_t lds_bytes(int, int) { return 0; }
    __device__ __forceinline__ void prepare(int lane) const
    {
        if constexpr (DIRECT) {
            int4_fill_pairs(pairs, lane, 64);
            __syncthreads();
        }
    }
    __device__ __forceinline__ void many(uint64_t mask, uint32_t id_lane, int lane, float *out) const
    {
        if (!((mask >> lane) & 1)) return;
        if constexpr (DIRECT)
            out[lane] = int4_l2_direct(qv, rows + static_cast<int64_t>(id_lane) * (dim >> 1), dim, mn, diff, pairs);
        else
            out[lane] = int4_l2_precomputed(qv, rows + static_cast<int64_t>(id_lane) * ((dim + 1) / 2), dim, table);
    }
    __device__ __forceinline__ bool risk(int lane) const
    {
        bool bad = false;
        float vm = 0.0f;
        if (mn && diff) {
            for (int j = lane; j < dim; j += 64) {
                bad = bad || !is_finite_f32(mn[j]) || !is_finite_f32(diff[j]);
                vm = fmaxf(vm, fabsf(mn[j]) + fabsf(diff[j]));
            }
        } else {
            for (int j = lane; j < dim * 16; j += 64) {  // (the lookup table holds the decoded values)
                bad = bad || !is_finite_f32(table[j]);
                vm = fmaxf(vm, fabsf(table[j]));
            }
        }
        return walk_risk(qv, dim, bad, vm, false, lane);
    }
};

__device__ inline float rq_formula_g(float qn, float yn, float dimf, float hamming)
{
    const float t1 = qn - yn;
    const float t1sq = t1 * t1;
    float t2 = 4.0f * qn;
    t2 = t2 * yn;
    t2 = t2 / dimf;
    t2 = t2 * hamming;
    return t1sq + t2;
}

struct VamanaRaBitQScorer {  // rabitq.go:119-176 from the query's code qc (rq_nb sign bytes, then its norm), one node per lane
    const uint8_t *rows, *qc;
    const float *qv, *absmax;
    // the query's sign words in LDS (broadcast reads — as scalar loads each one was a round trip the pass waited out), an LDS
    // pointer by type: through a generic one the unrolled loops lose their 128-bit reads and the instances their eighth wave
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    lds_u32 *qw;
    float qn;
    int nb, dim;
    __host__ __device__ static constexpr size_t lds_bytes(int, int rq_nb) { return rq_nb; }
    __device__ __forceinline__ static float norm_of(const uint8_t *qc, int nb)  // the float after the code's sign bytes
    {
        return __uint_as_float(qc[nb] | (qc[nb + 1] << 8) | (qc[nb + 2] << 16) | (static_cast<uint32_t>(qc[nb + 3]) << 24));
    }
    __device__ __forceinline__ void prepare(int lane) const
    {
        for (int i = lane; i < (nb >> 2); i += 64) qw[i] = reinterpret_cast<const uint32_t *>(qc)[i];  // (qcodes rows are 4-byte aligned)
        __syncthreads();
    }
    __device__ __forceinline__ void many(uint64_t mask, uint32_t id_lane, int lane, float *out) const
    {
        if (!((mask >> lane) & 1)) return;
        // rows are nb + 4 bytes with nb a multiple of 8: every row is 4-byte aligned, so the bits and the norm are read as
        // dwords, 8 loads in flight at a time
        const uint32_t *cw = reinterpret_cast<const uint32_t *>(rows + static_cast<int64_t>(id_lane) * (nb + 4));
        const int nw = nb >> 2;
        int h = 0;
        int b0 = 0;
        for (; b0 + 8 <= nw; b0 += 8) {
            uint32_t x[8];
#pragma unroll
            for (int u = 0; u < 8; u++) x[u] = cw[b0 + u];
#pragma unroll
            for (int u = 0; u < 8; u++) h += __popc(x[u] ^ qw[b0 + u]);
        }
        for (; b0 < nw; b0++) h += __popc(cw[b0] ^ qw[b0]);
        const uint32_t yb = cw[nw];
        out[lane] = rq_formula_g(qn, __uint_as_float(yb), static_cast<float>(dim), static_cast<float>(h));
    }
    __device__ __forceinline__ bool risk(int lane) const  // 4 |q| |y| overflowing next to a Hamming distance of 0
    {
        bool bad = false;
        for (int j = lane; j < dim; j += 64) bad = bad || !is_finite_f32(qv[j]);
        const float ma = absmax[0];
        return bad || !is_finite_f32(qn) || !is_finite_f32(ma) || !(4.0f * fabsf(qn) * ma < 1e38f) || !(score_bound(fabsf(qn), ma, false) < 1e38f);
    }
};

template <int kind>
struct VamanaScorer {  // the two PQ kinds are the HNSW walk's scorer: one copy of ComputeAsymmetricDistance
    using type = std::conditional_t<kind == kVamanaF32, VamanaF32Scorer,
                 std::conditional_t<kind == kVamanaPQ || kind == kVamanaPQDirect, PqScorerT<kind == kVamanaPQDirect>,
                 std::conditional_t<kind == kVamanaRaBitQ, VamanaRaBitQScorer, VamanaInt4Scorer<kind == kVamanaInt4Direct>>>>;
};

}  // namespace vg
