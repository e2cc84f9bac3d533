// v_mfma_i32_32x32x32_i8 on gfx950: the operand and result lane maps the RaBitQ nomination GEMM (k_rabitq_nominate.hip) relies on,
// checked with exact integer data and an ASYMMETRIC B (a symmetric one hides a transposed result), and the sign-bit expansion
// (rn_expand16, vg_rabitq.hpp) end to end: 32 x 32 Hamming distances over 128 bits from four MFMAs against the popcount.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../vecgo_amd/csrc -I../../include mfma_i8_probe.hip -o mfma_i8_probe && ./mfma_i8_probe
// Prints "maps ok" / "hamming ok" and exits 0, or the first disagreements and exits 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vg_rabitq.hpp"

#define CK(x)                                             \
    do {                                                  \
        hipError_t e = (x);                               \
        if (e != hipSuccess) {                            \
            printf("%s: %s\n", #x, hipGetErrorString(e)); \
            exit(1);                                      \
        }                                                 \
    } while (0)

typedef int i4 __attribute__((ext_vector_type(4)));
typedef int i16 __attribute__((ext_vector_type(16)));

// A [32][32] row-major (row m, k), B [32][32] (k, column n), C [32][32] (m, n): lane l holds A[l & 31][16 (l >> 5) + j] and
// B[16 (l >> 5) + j][l & 31] in byte j of its 16, and C[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31] in result register r.
__global__ void maps_kernel(const int8_t *a, const int8_t *b, int *c)
{
    const int l = threadIdx.x;
    union { i4 v; int8_t e[16]; } fa, fb;
    for (int j = 0; j < 16; j++) {
        fa.e[j] = a[(l & 31) * 32 + 16 * (l >> 5) + j];
        fb.e[j] = b[(16 * (l >> 5) + j) * 32 + (l & 31)];
    }
    i16 acc;
    for (int r = 0; r < 16; r++) acc[r] = 0;
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa.v, fb.v, acc, 0, 0, 0);
    for (int r = 0; r < 16; r++) c[((r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * 32 + (l & 31)] = acc[r];
}

// rows [32] and queries [32] of 128 sign bits (uint4 each): h[row][query] the way the GEMM forms it
__global__ void hamming_kernel(const uint4 *rows, const uint4 *queries, int *h)
{
    const int l = threadIdx.x;
    const uint4 rw = rows[l & 31], qw = queries[l & 31];
    const uint32_t r32[4] = {rw.x, rw.y, rw.z, rw.w}, q32[4] = {qw.x, qw.y, qw.z, qw.w};
    i16 acc;
    for (int r = 0; r < 16; r++) acc[r] = 0;
    for (int kk = 0; kk < 4; kk++) {
        const int ch = 2 * kk + (l >> 5);  // the 16-bit chunk of the 128 bits this lane half carries
        const uint4 ea = vg::rn_expand16((r32[ch >> 1] >> (16 * (ch & 1))) & 0xFFFFu), eb = vg::rn_expand16((q32[ch >> 1] >> (16 * (ch & 1))) & 0xFFFFu);
        const i4 fa = {int(ea.x), int(ea.y), int(ea.z), int(ea.w)}, fb = {int(eb.x), int(eb.y), int(eb.z), int(eb.w)};
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
    }
    for (int r = 0; r < 16; r++) h[((r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * 32 + (l & 31)] = (128 - acc[r]) >> 1;
}

int main()
{
    int bad = 0;
    {
        std::vector<int8_t> a(1024), b(1024);
        for (int m = 0; m < 32; m++)
            for (int k = 0; k < 32; k++) a[m * 32 + k] = int8_t((m * 3 + k * 5) % 11 - 5);
        for (int k = 0; k < 32; k++)
            for (int n = 0; n < 32; n++) b[k * 32 + n] = int8_t((k * 7 + n * 13 + k * n) % 9 - 4 + (n > k ? 3 : 0));  // B[k][n] != B[n][k]
        int8_t *da, *db;
        int *dc;
        CK(hipMalloc(&da, 1024)); CK(hipMalloc(&db, 1024)); CK(hipMalloc(&dc, 4096));
        CK(hipMemcpy(da, a.data(), 1024, hipMemcpyHostToDevice)); CK(hipMemcpy(db, b.data(), 1024, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(maps_kernel, dim3(1), dim3(64), 0, 0, da, db, dc);
        std::vector<int> c(1024);
        CK(hipMemcpy(c.data(), dc, 4096, hipMemcpyDeviceToHost));
        for (int m = 0; m < 32; m++)
            for (int n = 0; n < 32; n++) {
                int want = 0;
                for (int k = 0; k < 32; k++) want += int(a[m * 32 + k]) * int(b[k * 32 + n]);
                if (c[m * 32 + n] != want && bad++ < 8) printf("maps: C[%d][%d] = %d, want %d\n", m, n, c[m * 32 + n], want);
            }
        if (!bad) printf("maps ok\n");
    }
    const int bad_maps = bad;
    {
        std::vector<uint32_t> rows(128), queries(128);
        uint32_t x = 12345;
        auto next = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
        for (auto &w : rows) w = next();
        for (auto &w : queries) w = next() & next();  // (sparser: Hamming distances away from 64)
        for (int j = 0; j < 4; j++) rows[j] = 0, rows[4 + j] = 0xFFFFFFFFu, queries[8 + j] = rows[12 + j];
        uint4 *dr, *dq;
        int *dh;
        CK(hipMalloc(&dr, 512)); CK(hipMalloc(&dq, 512)); CK(hipMalloc(&dh, 4096));
        CK(hipMemcpy(dr, rows.data(), 512, hipMemcpyHostToDevice)); CK(hipMemcpy(dq, queries.data(), 512, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(hamming_kernel, dim3(1), dim3(64), 0, 0, dr, dq, dh);
        std::vector<int> h(1024);
        CK(hipMemcpy(h.data(), dh, 4096, hipMemcpyDeviceToHost));
        for (int m = 0; m < 32; m++)
            for (int n = 0; n < 32; n++) {
                int want = 0;
                for (int j = 0; j < 4; j++) want += __builtin_popcount(rows[m * 4 + j] ^ queries[n * 4 + j]);
                if (h[m * 32 + n] != want && bad++ < 16) printf("hamming: h[row %d][query %d] = %d, want %d\n", m, n, h[m * 32 + n], want);
            }
        if (bad == bad_maps) printf("hamming ok\n");
    }
    return bad ? 1 : 0;
}
