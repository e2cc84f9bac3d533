// k_sq8.hip — the 8-bit scalar quantizer:
//   quantization.ScalarQuantizer   internal/quantization/quantizer.go:27-250
//   simd.Sq8uL2BatchPerDimension   internal/simd/src/sq8_avx512.c:59-103
// (the SQ8 codes of an index and their search: k_sq8_scan.hip)
// Numerics contract (sq8_avx512.c): per row 16 lane accumulators over 16-element blocks,
//   rec = fma(float(code), invScale[j], min[j]); diff = q[j] - rec; sum[l] = fma(diff, diff, sum[l])
// then the _mm512_reduce_add_ps tree and an FMA-contracted scalar tail.  Here ONE GPU lane owns a
// row and keeps the 16 accumulators in registers, so a wave scores 64 rows at a time (vg_sq8_row.hpp).
#include <algorithm>

#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"
#include "vg_sq8_row.hpp"

namespace vg {

// ---- Train (quantizer.go:127-180) ----------------------------------------------------------------
// stage 1 (INT4's Train shares it: launch_dim_minmax): thread = (row chunk, dimension): min / max over the chunk's rows (order-free, exact)
__global__ void dim_minmax_kernel(const float *__restrict__ v, int64_t n, int dim, int chunks,
                                  float *__restrict__ pmin, float *__restrict__ pmax)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (d >= dim) return;
    const int64_t r0 = n * c / chunks, r1 = n * (c + 1) / chunks;
    float mn = kF32Max, mx = -kF32Max;
    int64_t i = r0;
    for (; i + 8 <= r1; i += 8) {  // 8 rows in flight per thread; the data is read once
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = __builtin_nontemporal_load(v + (i + u) * dim + d);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (x[u] < mn) mn = x[u];
            if (x[u] > mx) mx = x[u];
        }
    }
    for (; i < r1; i++) {
        const float x = v[i * dim + d];
        if (x < mn) mn = x;
        if (x > mx) mx = x;
    }
    pmin[static_cast<int64_t>(c) * dim + d] = mn;
    pmax[static_cast<int64_t>(c) * dim + d] = mx;
}

// stage 2 + scales.  from_train: a constant dimension gets max = min + 1e-6 (quantizer.go:168-170);
// SetBounds instead zeroes both scales when max - min < 1e-9 (quantizer.go:64-72).
__global__ void sq8_finish_kernel(const float *__restrict__ pmin, const float *__restrict__ pmax, int chunks,
                                  int dim, bool from_train, float *__restrict__ mins, float *__restrict__ maxs,
                                  float *__restrict__ scales, float *__restrict__ inv)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= dim) return;
    float mn, mx;
    if (from_train) {
        mn = kF32Max;
        mx = -kF32Max;
        for (int c = 0; c < chunks; c++) {
            const float a = pmin[static_cast<int64_t>(c) * dim + d], b = pmax[static_cast<int64_t>(c) * dim + d];
            if (a < mn) mn = a;
            if (b > mx) mx = b;
        }
        if (mn == mx) mx = mn + 1e-6f;
        const float range = mx - mn;
        scales[d] = 255.0f / range;
        inv[d] = range / 255.0f;
    } else {
        mn = pmin[d];
        mx = pmax[d];
        const float diff = mx - mn;
        if (diff < 1e-9f) {
            scales[d] = 0.0f;
            inv[d] = 0.0f;
        } else {
            scales[d] = 255.0f / diff;
            inv[d] = diff / 255.0f;
        }
    }
    mins[d] = mn;
    maxs[d] = mx;
}

// stage 1 of a Train (SQ8 here, INT4 in k_int4.hip) over device rows: pmin / pmax [chunks][dim] for the finish kernel
int32_t launch_dim_minmax(const float *d_rows, int64_t n, int dim, DevTmp<float> &pmin, DevTmp<float> &pmax, int &chunks,
                          hipStream_t st)
{
    chunks = static_cast<int>(std::min<int64_t>(n, 1024));
    VG_TRY(pmin.init(static_cast<size_t>(chunks) * dim, st));
    VG_TRY(pmax.init(static_cast<size_t>(chunks) * dim, st));
    VG_LAUNCH(dim_minmax_kernel, dim3((dim + 255) / 256, chunks), dim3(256), 0, st, d_rows, n, dim, chunks, pmin.ptr, pmax.ptr);
    return VG_OK;
}

// ---- EncodeInto / DecodeInto (quantizer.go:198-250): thread per element -----------------------------
__global__ void sq8_encode_kernel(const float *__restrict__ v, int64_t total, int dim,
                                  const float *__restrict__ mins, const float *__restrict__ maxs,
                                  const float *__restrict__ scales, uint8_t *__restrict__ out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int d = static_cast<int>(i % dim);
    float val = v[i];
    const float mn = mins[d], mx = maxs[d];
    if (val < mn)
        val = mn;
    else if (val > mx)
        val = mx;
    const float normalized = (val - mn) * scales[d];
    const float r = normalized + 0.5f;
    out[i] = static_cast<uint8_t>(static_cast<int>(r));  // Go uint8(float32): truncation
}

__global__ void sq8_decode_kernel(const uint8_t *__restrict__ codes, int64_t total, int dim,
                                  const float *__restrict__ mins, const float *__restrict__ inv,
                                  float *__restrict__ out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int d = static_cast<int>(i % dim);
    const float t = static_cast<float>(codes[i]) * inv[d];
    out[i] = t + mins[d];
}

// The element kernels above spend their time on `i % dim` (a 64-bit division per element): 1.6 - 1.75 TB/s.  dim % 4
// == 0 and 16-byte aligned buffers: a thread owns four consecutive dimensions (its parameters loaded once) and walks
// kRowsPerThread rows — no division, 16-byte loads / stores, the same operations per element.
__global__ __launch_bounds__(256) void sq8_encode4_kernel(const float *__restrict__ v, int64_t n, int dim,
                                                          const float *__restrict__ mins, const float *__restrict__ maxs,
                                                          const float *__restrict__ scales, uint8_t *__restrict__ out, int rpt)
{
    const int cg = blockIdx.x * blockDim.x + threadIdx.x;
    if (cg * 4 >= dim) return;
    const float4 mn = *reinterpret_cast<const float4 *>(mins + cg * 4), mx = *reinterpret_cast<const float4 *>(maxs + cg * 4),
                 sc = *reinterpret_cast<const float4 *>(scales + cg * 4);
    const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpt;
    auto enc = [](float val, float lo, float hi, float s) -> uint32_t {
        if (val < lo)
            val = lo;
        else if (val > hi)
            val = hi;
        const float normalized = (val - lo) * s;
        const float r = normalized + 0.5f;
        return static_cast<uint32_t>(static_cast<uint8_t>(static_cast<int>(r)));  // Go uint8(float32): truncation
    };
    for (int64_t row = r0; row < r0 + rpt && row < n; row++) {
        const float4 x = *reinterpret_cast<const float4 *>(v + row * dim + cg * 4);
        const uint32_t w = enc(x.x, mn.x, mx.x, sc.x) | (enc(x.y, mn.y, mx.y, sc.y) << 8) | (enc(x.z, mn.z, mx.z, sc.z) << 16) |
                           (enc(x.w, mn.w, mx.w, sc.w) << 24);
        *reinterpret_cast<uint32_t *>(out + row * dim + cg * 4) = w;
    }
}
__global__ __launch_bounds__(256) void sq8_decode4_kernel(const uint8_t *__restrict__ codes, int64_t n, int dim,
                                                          const float *__restrict__ mins, const float *__restrict__ inv,
                                                          float *__restrict__ out, int rpt)
{
    const int cg = blockIdx.x * blockDim.x + threadIdx.x;
    if (cg * 4 >= dim) return;
    const float4 mn = *reinterpret_cast<const float4 *>(mins + cg * 4), iv = *reinterpret_cast<const float4 *>(inv + cg * 4);
    const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpt;
    for (int64_t row = r0; row < r0 + rpt && row < n; row++) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(codes + row * dim + cg * 4);
        float4 o;
        float t;
        t = static_cast<float>(w & 0xFFu) * iv.x;
        o.x = t + mn.x;
        t = static_cast<float>((w >> 8) & 0xFFu) * iv.y;
        o.y = t + mn.y;
        t = static_cast<float>((w >> 16) & 0xFFu) * iv.z;
        o.z = t + mn.z;
        t = static_cast<float>(w >> 24) * iv.w;
        o.w = t + mn.w;
        *reinterpret_cast<float4 *>(out + row * dim + cg * 4) = o;
    }
}

// L2DistanceBatch on the reference layout (codes n*dim): lane per row, 16 bytes at a time.  The
// interface path for small batches (the reference calls it with 256 rows, flat/segment.go:487,550).
__global__ __launch_bounds__(256) void sq8_l2_batch_kernel(const float *__restrict__ query,
                                                           const uint8_t *__restrict__ codes, int64_t n, int dim,
                                                           const float *__restrict__ mins,
                                                           const float *__restrict__ inv, float *__restrict__ out)
{
    const int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint8_t *cp = codes + row * dim;
    float acc[16];
#pragma unroll
    for (int l = 0; l < 16; l++) acc[l] = 0.0f;
    int j = 0;
    for (; j + 16 <= dim; j += 16) {
        uint32_t w[4];
#pragma unroll
        for (int t = 0; t < 4; t++)  // rows are only byte-aligned
            w[t] = cp[j + 4 * t] | (cp[j + 4 * t + 1] << 8) | (cp[j + 4 * t + 2] << 16) |
                   (static_cast<uint32_t>(cp[j + 4 * t + 3]) << 24);
        sq8_block16(acc, make_uint4(w[0], w[1], w[2], w[3]), query + j, mins + j, inv + j);
    }
    float total = reduce16_regs(acc);
    for (; j < dim; j++) {
        const float rec = __builtin_fmaf(static_cast<float>(cp[j]), inv[j], mins[j]);
        const float diff = query[j] - rec;
        total = __builtin_fmaf(diff, diff, total);
    }
    out[row] = total;
}

// The same distances as a streaming scan (dim % 128 == 0, 16-byte aligned codes): the kernel above reads its row a byte
// at a time at a dim-byte stride (1.07 TB/s of codes at dim 768).  Here a wave takes 64 rows, 128-byte pieces of them
// arrive as whole lines (8 lanes per row; the next piece in flight while this one is scored) and are turned through
// the wave's LDS (row stride 144 bytes = 16 x 9: conflict-free ds_read_b128), each lane then walks ITS row with
// sq8_block16 — the same 16 accumulators in the same order.
constexpr int kSqTurnWaves = 4;
constexpr int kSqTurnStride = 144;
__global__ __launch_bounds__(kSqTurnWaves * 64) void sq8_l2_batch_turn_kernel(const float *__restrict__ query,
                                                                              const uint8_t *__restrict__ codes, int64_t n,
                                                                              int dim, const float *__restrict__ mins,
                                                                              const float *__restrict__ inv,
                                                                              float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage_all[kSqTurnWaves][64 * kSqTurnStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = (static_cast<int64_t>(blockIdx.x) * kSqTurnWaves + wave) * 64;
    if (row0 >= n) return;
    unsigned char *stage = stage_all[wave];
    const int r = lane >> 3, part = lane & 7;
    auto row_ptr = [&](int k) {
        const int64_t row = row0 + r + 8 * k < n ? row0 + r + 8 * k : n - 1;  // past n: row n - 1 again, not stored
        return codes + row * dim + part * 16;
    };
    const uint8_t *s0 = row_ptr(0), *s1 = row_ptr(1), *s2 = row_ptr(2), *s3 = row_ptr(3), *s4 = row_ptr(4),
                  *s5 = row_ptr(5), *s6 = row_ptr(6), *s7 = row_ptr(7);
#define VG_SQ_LD(P, OFF) load_stream(reinterpret_cast<const uint4 *>((P) + (OFF)))
    uint4 u0 = VG_SQ_LD(s0, 0), u1 = VG_SQ_LD(s1, 0), u2 = VG_SQ_LD(s2, 0), u3 = VG_SQ_LD(s3, 0), u4 = VG_SQ_LD(s4, 0),
          u5 = VG_SQ_LD(s5, 0), u6 = VG_SQ_LD(s6, 0), u7 = VG_SQ_LD(s7, 0);
    float acc[16];
#pragma unroll
    for (int l = 0; l < 16; l++) acc[l] = 0.0f;
    unsigned char *wr = stage + r * kSqTurnStride + part * 16;
    for (int cb0 = 0; cb0 < dim; cb0 += 128) {
        *reinterpret_cast<uint4 *>(wr) = u0;
        *reinterpret_cast<uint4 *>(wr + 8 * kSqTurnStride) = u1;
        *reinterpret_cast<uint4 *>(wr + 16 * kSqTurnStride) = u2;
        *reinterpret_cast<uint4 *>(wr + 24 * kSqTurnStride) = u3;
        *reinterpret_cast<uint4 *>(wr + 32 * kSqTurnStride) = u4;
        *reinterpret_cast<uint4 *>(wr + 40 * kSqTurnStride) = u5;
        *reinterpret_cast<uint4 *>(wr + 48 * kSqTurnStride) = u6;
        *reinterpret_cast<uint4 *>(wr + 56 * kSqTurnStride) = u7;
        const int nxt = cb0 + 128 < dim ? cb0 + 128 : cb0;  // (the last piece again: unused)
        u0 = VG_SQ_LD(s0, nxt);
        u1 = VG_SQ_LD(s1, nxt);
        u2 = VG_SQ_LD(s2, nxt);
        u3 = VG_SQ_LD(s3, nxt);
        u4 = VG_SQ_LD(s4, nxt);
        u5 = VG_SQ_LD(s5, nxt);
        u6 = VG_SQ_LD(s6, nxt);
        u7 = VG_SQ_LD(s7, nxt);
#undef VG_SQ_LD
        for (int piece = 0; piece < 8; piece++) {
            const uint4 c = *reinterpret_cast<const uint4 *>(stage + lane * kSqTurnStride + piece * 16);
            const int j = cb0 + piece * 16;
            sq8_block16(acc, c, query + j, mins + j, inv + j);
        }
    }
    const float total = reduce16_regs(acc);
    if (row0 + lane < n) out[row0 + lane] = total;
}

}  // namespace vg

// ---- C ABI --------------------------------------------------------------------------------------------
VG_API int32_t vg_sq8_create(vg_ctx *ctx, int32_t dim, vg_sq8 **out)
{
    VG_CHECK(out, VG_ERR_INVALID_ARG, "vg_sq8_create: out is NULL");
    *out = nullptr;
    VG_CHECK(ctx, VG_ERR_INVALID_ARG, "vg_sq8_create: ctx is NULL");
    VG_CHECK(dim > 0, VG_ERR_INVALID_ARG, "vg_sq8_create: dim must be positive");
    VG_HIP(hipSetDevice(ctx->device));
    vg_sq8 *sq = new vg_sq8;
    sq->ctx = ctx;
    sq->dim = dim;
    float *block = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&block), sizeof(float) * 4 * static_cast<size_t>(dim));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete sq;
        vg::set_error("vg_sq8_create: hipMalloc failed: %s", hipGetErrorString(e));
        return VG_ERR_HIP;
    }
    sq->d_mins = block;
    sq->d_maxs = block + dim;
    sq->d_scales = block + 2 * dim;
    sq->d_inv = block + 3 * dim;
    *out = sq;
    return VG_OK;
}

VG_API int32_t vg_sq8_destroy(vg_sq8 *sq)
{
    if (!sq) return VG_OK;
    (void)hipSetDevice(sq->ctx->device);
    if (sq->d_mins) (void)hipFree(sq->d_mins);
    delete sq;
    return VG_OK;
}

VG_API int32_t vg_sq8_is_trained(vg_sq8 *sq) { return sq && sq->trained ? 1 : 0; }

VG_API int32_t vg_sq8_train(vg_sq8 *sq, const float *vectors, int64_t n, void *stream)
{
    VG_CHECK(sq, VG_ERR_INVALID_ARG, "vg_sq8_train: NULL quantizer");
    VG_CHECK(n > 0 && vectors, VG_ERR_INVALID_ARG, "no vectors provided for training");  // quantizer.go:128-130
    VG_HIP(hipSetDevice(sq->ctx->device));
    hipStream_t st = vg::pick_stream(sq->ctx, stream);
    const int dim = sq->dim;
    vg::DevIn<float> v;
    VG_TRY(v.init(vectors, static_cast<size_t>(n) * dim, st));
    int chunks;
    vg::DevTmp<float> pmin, pmax;
    VG_TRY(vg::launch_dim_minmax(v.ptr, n, dim, pmin, pmax, chunks, st));
    VG_LAUNCH(vg::sq8_finish_kernel, dim3((dim + 255) / 256), dim3(256), 0, st, pmin.ptr, pmax.ptr, chunks, dim,
              true, sq->d_mins, sq->d_maxs, sq->d_scales, sq->d_inv);
    VG_HIP(hipStreamSynchronize(st));
    sq->trained = true;
    return VG_OK;
}

VG_API int32_t vg_sq8_set_bounds(vg_sq8 *sq, const float *mins, const float *maxs)
{
    VG_CHECK(sq, VG_ERR_INVALID_ARG, "vg_sq8_set_bounds: NULL quantizer");
    VG_CHECK(mins && maxs, VG_ERR_INVALID_ARG, "vg_sq8_set_bounds: NULL bounds");
    VG_HIP(hipSetDevice(sq->ctx->device));
    hipStream_t st = sq->ctx->stream;
    vg::DevIn<float> a, b;
    VG_TRY(a.init(mins, static_cast<size_t>(sq->dim), st));
    VG_TRY(b.init(maxs, static_cast<size_t>(sq->dim), st));
    VG_LAUNCH(vg::sq8_finish_kernel, dim3((sq->dim + 255) / 256), dim3(256), 0, st, a.ptr, b.ptr, 1, sq->dim, false,
              sq->d_mins, sq->d_maxs, sq->d_scales, sq->d_inv);
    VG_HIP(hipStreamSynchronize(st));
    sq->trained = true;
    return VG_OK;
}

VG_API int32_t vg_sq8_get_params(vg_sq8 *sq, float *mins, float *maxs, float *scales, float *inv_scales)
{
    VG_CHECK(sq, VG_ERR_INVALID_ARG, "vg_sq8_get_params: NULL quantizer");
    VG_CHECK(sq->trained, VG_ERR_NOT_TRAINED, "ScalarQuantizer not trained");
    VG_HIP(hipSetDevice(sq->ctx->device));
    hipStream_t st = sq->ctx->stream;
    const size_t b = sizeof(float) * static_cast<size_t>(sq->dim);
    if (mins) VG_HIP(hipMemcpyAsync(mins, sq->d_mins, b, hipMemcpyDefault, st));
    if (maxs) VG_HIP(hipMemcpyAsync(maxs, sq->d_maxs, b, hipMemcpyDefault, st));
    if (scales) VG_HIP(hipMemcpyAsync(scales, sq->d_scales, b, hipMemcpyDefault, st));
    if (inv_scales) VG_HIP(hipMemcpyAsync(inv_scales, sq->d_inv, b, hipMemcpyDefault, st));
    VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}

VG_API int32_t vg_sq8_encode(vg_sq8 *sq, const float *vectors, int64_t n, uint8_t *codes, void *stream)
{
    VG_CHECK(sq, VG_ERR_INVALID_ARG, "vg_sq8_encode: NULL quantizer");
    VG_CHECK(sq->trained, VG_ERR_NOT_TRAINED, "ScalarQuantizer not trained");  // quantizer.go:184-186
    VG_CHECK(n >= 0, VG_ERR_INVALID_ARG, "vg_sq8_encode: n < 0");
    if (n == 0) return VG_OK;
    VG_CHECK(vectors && codes, VG_ERR_INVALID_ARG, "vg_sq8_encode: NULL buffer");
    VG_HIP(hipSetDevice(sq->ctx->device));
    hipStream_t st = vg::pick_stream(sq->ctx, stream);
    const int64_t total = n * sq->dim;
    vg::DevIn<float> v;
    vg::DevOut<uint8_t> c;
    VG_TRY(v.init(vectors, static_cast<size_t>(total), st, vg::kAnyAlign));
    VG_TRY(c.init(codes, static_cast<size_t>(total), st, vg::kAnyAlign));
    const vg::RowWalk walk(n);
    if (sq->dim % 4 == 0 && vg::aligned16(v.ptr, c.ptr))
        VG_LAUNCH(vg::sq8_encode4_kernel, dim3((sq->dim / 4 + 255) / 256, walk.blocks_y),
                  dim3(256), 0, st, v.ptr, n, sq->dim, sq->d_mins, sq->d_maxs, sq->d_scales, c.ptr, walk.rpt);
    else
        VG_LAUNCH(vg::sq8_encode_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st, v.ptr, total,
                  sq->dim, sq->d_mins, sq->d_maxs, sq->d_scales, c.ptr);
    VG_TRY(c.finish());
    return VG_OK;
}

VG_API int32_t vg_sq8_decode(vg_sq8 *sq, const uint8_t *codes, int64_t n, float *out, void *stream)
{
    VG_CHECK(sq, VG_ERR_INVALID_ARG, "vg_sq8_decode: NULL quantizer");
    VG_CHECK(sq->trained, VG_ERR_NOT_TRAINED, "ScalarQuantizer not trained");
    VG_CHECK(n >= 0, VG_ERR_INVALID_ARG, "vg_sq8_decode: n < 0");
    if (n == 0) return VG_OK;
    VG_CHECK(codes && out, VG_ERR_INVALID_ARG, "vg_sq8_decode: NULL buffer");
    VG_HIP(hipSetDevice(sq->ctx->device));
    hipStream_t st = vg::pick_stream(sq->ctx, stream);
    const int64_t total = n * sq->dim;
    vg::DevIn<uint8_t> c;
    vg::DevOut<float> o;
    VG_TRY(c.init(codes, static_cast<size_t>(total), st, vg::kAnyAlign));
    VG_TRY(o.init(out, static_cast<size_t>(total), st, vg::kAnyAlign));
    const vg::RowWalk walk(n);
    if (sq->dim % 4 == 0 && vg::aligned16(c.ptr, o.ptr))
        VG_LAUNCH(vg::sq8_decode4_kernel, dim3((sq->dim / 4 + 255) / 256, walk.blocks_y),
                  dim3(256), 0, st, c.ptr, n, sq->dim, sq->d_mins, sq->d_inv, o.ptr, walk.rpt);
    else
        VG_LAUNCH(vg::sq8_decode_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st, c.ptr, total,
                  sq->dim, sq->d_mins, sq->d_inv, o.ptr);
    VG_TRY(o.finish());
    return VG_OK;
}

VG_API int32_t vg_sq8_l2_distance_batch(vg_sq8 *sq, const float *query, const uint8_t *codes, int64_t n,
                                        float *out, void *stream)
{
    VG_CHECK(sq, VG_ERR_INVALID_ARG, "vg_sq8_l2_distance_batch: NULL quantizer");
    VG_CHECK(sq->trained, VG_ERR_NOT_TRAINED, "ScalarQuantizer not trained");
    VG_CHECK(n >= 0, VG_ERR_INVALID_ARG, "vg_sq8_l2_distance_batch: n < 0");
    if (n == 0) return VG_OK;
    VG_CHECK(query && codes && out, VG_ERR_INVALID_ARG, "vg_sq8_l2_distance_batch: NULL buffer");
    VG_HIP(hipSetDevice(sq->ctx->device));
    hipStream_t st = vg::pick_stream(sq->ctx, stream);
    vg::DevIn<float> q;
    vg::DevIn<uint8_t> c;
    vg::DevOut<float> o;
    VG_TRY(q.init(query, static_cast<size_t>(sq->dim), st));
    VG_TRY(c.init(codes, static_cast<size_t>(n) * sq->dim, st, vg::kAnyAlign));
    VG_TRY(o.init(out, static_cast<size_t>(n), st));
    if (sq->dim % 128 == 0 && vg::aligned16(c.ptr))
        VG_LAUNCH(vg::sq8_l2_batch_turn_kernel,
                  dim3(static_cast<unsigned>(((n + 63) / 64 + vg::kSqTurnWaves - 1) / vg::kSqTurnWaves)),
                  dim3(vg::kSqTurnWaves * 64), 0, st, q.ptr, c.ptr, n, sq->dim, sq->d_mins, sq->d_inv, o.ptr);
    else
        VG_LAUNCH(vg::sq8_l2_batch_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, q.ptr, c.ptr, n,
                  sq->dim, sq->d_mins, sq->d_inv, o.ptr);
    VG_TRY(o.finish());
    return VG_OK;
}
