// vg_rabitq.hpp — what the RaBitQ translation units share (k_rabitq.hip: the codec and the scans; k_rabitq_nominate.hip: the batch
// search through an int8 matrix-core nomination, vg_index_enable_rabitq_nomination): the distance formula, the Hamming distance of
// two codes, the nomination's screen and the host functions one unit defines and the other calls.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "vg_device.hpp"
#include "vg_internal.hpp"

namespace vg {

__host__ __device__ inline int rq_words(int dim) { return (dim + 63) / 64; }

__device__ inline float rq_formula(float qn, float yn, float dimf, float hamming)
{
    // rabitq.go:170-175, fp32, left to right, no fusion
    const float t1 = qn - yn;
    const float t1sq = t1 * t1;
    float t2 = 4.0f * qn;
    t2 = t2 * yn;
    t2 = t2 / dimf;
    t2 = t2 * hamming;
    return t1sq + t2;
}

// popcount(a ^ c) over nbytes bytes: dwords, 8 loads in flight at a time, when both are 4-byte aligned
__device__ __forceinline__ int hamming_bytes(const uint8_t *__restrict__ a, const uint8_t *__restrict__ c, int64_t nbytes)
{
    int h = 0;
    int64_t b = 0;
    if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(c)) & 3) == 0) {
        const uint32_t *aw = reinterpret_cast<const uint32_t *>(a), *cw = reinterpret_cast<const uint32_t *>(c);
        const int64_t nw = nbytes >> 2;
        int64_t w = 0;
        for (; w + 8 <= nw; w += 8) {
            uint32_t x[8];
#pragma unroll
            for (int u = 0; u < 8; u++) x[u] = cw[w + u];
#pragma unroll
            for (int u = 0; u < 8; u++) h += __popc(x[u] ^ aw[w + u]);
        }
        for (; w < nw; w++) h += __popc(cw[w] ^ aw[w]);
        b = nw << 2;
    }
    for (; b < nbytes; b++) h += __popc(static_cast<unsigned>(a[b] ^ c[b]));
    return h;
}

// the norm a code carries behind its nb bytes of sign bits
__device__ __forceinline__ float rq_code_norm(const uint8_t *c, int nb)
{
    return __uint_as_float(c[nb] | (c[nb + 1] << 8) | (c[nb + 2] << 16) | (static_cast<uint32_t>(c[nb + 3]) << 24));
}

// ---- the nomination's screen ------------------------------------------------------------------------------------------------
// The GEMM's epilogue has the exact Hamming distance h of a (query, row) pair and decides whether the pair's exact score — rq_formula
// in the reference's operation order — may be <= the query's threshold tau.  It is CONSERVATIVE: every pair with rq_formula <= tau
// passes.  The exact formula divides once per pair; the screen multiplies instead:
//   t1sq = (qn - yn)^2                      exactly the reference's two operations
//   b    = RN(RN(4 qn) yn)                  exactly the reference's
//   c~   = RN(b * invd)                     invd = RN(1 / dim) moved one ulp towards zero (rq_screen_invd)
//   s~   = RN(t1sq + RN(c~ * h))
// and passes when s~ <= tau.  Round-to-nearest is monotone, and that is the whole proof: RN(1 / dim) is within half an ulp of
// 1 / dim, so invd < 1 / dim as real numbers; for b >= 0 (stored norms that are not negative; a query's norm is a square root)
// b invd <= b / dim, hence c~ = RN(b invd) <= RN(b / dim) = c, the reference's quotient — normal, subnormal or zero alike, no
// relative-error argument and so no absolute term; then RN(c~ h) <= RN(c h) for h >= 0 and s~ <= the exact score.  An infinite b
// gives the reference's own Inf / NaN.  NaN compares false: the pair is not listed, and a query whose scores may hold a NaN is
// replayed (vg_cand_replay.hpp) whatever was listed.  A NEGATIVE stored norm turns the inequality round (c~ > c): an index that
// holds one keeps the scan (rabitq_nomination_applies; vg_index_enable_rabitq_nomination looks once).  What the screen lists for
// nothing: pairs within an ulp or two of tau.  tests/test_rabitq_screen_bound_cpu.py restates this in numpy float32 against the
// oracle's distance.
inline float rq_screen_invd(int dim)
{
    const float r = 1.0f / static_cast<float>(dim);
    uint32_t u;
    std::memcpy(&u, &r, 4);
    u -= 1;  // (1 / dim >= 2^-13 for dim <= 8192: a normal number, and so is its neighbour)
    float out;
    std::memcpy(&out, &u, 4);
    return out;
}

// ---- the nomination's operands ----------------------------------------------------------------------------------------------
// 16 sign bits -> 16 int8: bit i set -> byte i = +1, clear -> -1
__device__ __forceinline__ uint4 rn_expand16(uint32_t b)
{
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t nib = (b >> (4 * j)) & 15u;
        const uint32_t t = (nib * 0x00204081u) & 0x01010101u;  // bit i of the nibble -> byte i (0 or 1)
        w[j] = __builtin_amdgcn_perm(0u, 0x000001FFu, t);       // byte 0 -> 0xFF (-1), byte 1 -> 0x01 (+1)
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- k_rabitq.hip -----------------------------------------------------------------------------------------------------------
// vg_search_rabitq's scan of nq device queries (encode, scan, merge; no NaN replay): ids / scores [nq * k]
int32_t rabitq_scan_batch(vg_index *idx, const float *q, int64_t nq, int k, uint8_t *qcodes, uint32_t *oid, float *osc, hipStream_t st);
// The threshold sample of the nomination: every 64th 64-row tile scored exactly by rabitq_scan_mq_kernel for cnt encoded queries;
// thr[q * sel_k + j] = the query's j-th best sampled score, +Inf past the sample's end.  partial: cnt * slices * sel_k keys.
int rabitq_sample_slices(const vg_index *idx, int64_t cnt);
int32_t launch_rabitq_sample(const vg_index *idx, const uint8_t *qcodes, int64_t cnt, int sel_k, int slices, uint64_t *partial, uint32_t *ids,
                             float *thr, hipStream_t st);
// ---- k_rabitq_nominate.hip --------------------------------------------------------------------------------------------------
bool rabitq_nomination_applies(const vg_index *idx, int64_t nq, int k);
// nomination, exact re-score and proof of nq device queries (qcodes: their codes); failed: the queries the caller scans
int32_t rabitq_nominated_pass(vg_index *idx, const uint8_t *qcodes, int64_t nq, int k, uint32_t *oid, float *osc, hipStream_t st,
                              std::vector<int> &failed);
int32_t rabitq_nomination_drop(vg_index *idx);

}  // namespace vg
