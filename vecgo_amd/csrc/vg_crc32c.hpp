// vg_crc32c.hpp — CRC-32C of pieces put together: the GF(2) arithmetic behind zlib's crc32_combine, for the Castagnoli
// polynomial (reflected 0x82F63B78; internal/hash/crc32c.go:15-17).  Host and device.
//   A CRC register is a polynomial over GF(2) of degree < 32, bit 31 the coefficient of x^0 (the reflected form).  Feeding k
//   zero bytes to a register multiplies it by x^(8k) mod P, and with init = xorout = 0xFFFFFFFF the CRCs of two pieces obey
//       crc(A || B) = crc(A) * x^(8 |B|)  ^  crc(B)
//   while the raw register (init 0, no final xor) R obeys the same rule and R(zeros) = 0:
//       crc(M) = R(M) ^ 0xFFFFFFFF * x^(8 |M|) ^ 0xFFFFFFFF
//   The device kernel (k_flat_build.hip) computes R of 16-byte pieces interleaved over the lanes; everything it needs beyond
//   the slicing tables is a product by a power of x.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define VG_CRC_HD __host__ __device__
#else
#define VG_CRC_HD
#endif

namespace vg {
namespace crc {

constexpr uint32_t kPoly = 0x82F63B78u;

// a * b mod P
VG_CRC_HD inline uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

// x^(8 * bytes) mod P: square and multiply (the order of x divides 2^32 - 1, so the exponent's bits past 32 wrap)
VG_CRC_HD inline uint32_t xpow8(uint64_t bytes)
{
    uint32_t sq = 0x00800000u;  // x^8
    uint32_t p = 0x80000000u;   // x^0
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) p = mulmod(sq, p);
        sq = mulmod(sq, sq);
    }
    return p;
}

// crc(A || B) from crc(A), crc(B), |B| — also the raw registers'
VG_CRC_HD inline uint32_t combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return mulmod(xpow8(len_b), crc_a) ^ crc_b; }

// crc(M) from the raw register R(M)
VG_CRC_HD inline uint32_t finish_raw(uint32_t raw, uint64_t len) { return raw ^ mulmod(xpow8(len), 0xFFFFFFFFu) ^ 0xFFFFFFFFu; }

}  // namespace crc
}  // namespace vg
