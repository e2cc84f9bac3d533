// vg_int4_plan.hpp — which kernel a one-query INT4 distance scan (vg_int4_l2_distance_batch, k_int4.hip) runs and in what
// launch shape.  HOST ONLY (no HIP): tests/cpp/host_mirror_test.cpp checks it at compile time, vg_int4_scan_plan hands it to
// a test, tests/scan_shapes.py restates it.
#pragma once

#include <cstdint>

namespace vg {

constexpr int kI4Waves = 4;         // int4_scan_kernel: waves (64-row tiles) per workgroup
constexpr int kI4Stride = 144;      // LDS bytes per staged row piece (128 + 16)
constexpr int kI4TabWaves = 12;     // int4_scan_tab_kernel: waves per workgroup, fewer when the table leaves less room
constexpr int kI4TabStride = 144;
constexpr int kI4TabMaxDim = 1024;
constexpr int kI4TabLds = 160 * 1024;
constexpr int kI4SmallGrid = 2;     // workgroups of the table scan under the test hook VG_INT4_SMALL_GRID

// the body int4_scan_kernel takes (the kernel branches on this very function): rows of whole 128-byte pieces
constexpr bool int4_whole_pieces(int row_bytes) { return (row_bytes & 127) == 0; }

enum Int4ScanKernel : int32_t {
    kI4Tab = 0,       // int4_scan_tab_kernel: persistent waves, the quantizer's value table in LDS
    kI4Pair128 = 1,   // int4_scan_kernel, int4_whole_pieces: 8 lanes per row, the next piece in flight
    kI4PairTail = 2,  // int4_scan_kernel, the other body: a last piece of 32, 64 or 96 bytes
    kI4Row = 3,       // int4_l2_batch_kernel / int4_l2_precomputed_kernel: a lane per row
};

struct Int4ScanPlan {
    int32_t kernel;  // Int4ScanKernel
    int32_t waves;   // per workgroup
    int64_t blocks;  // workgroups
    int64_t lds;     // dynamic LDS bytes (the table scan: table + staging; the others have none)
};

// n > 0 rows of `dim` dimensions; codes_aligned16: the codes' address is a multiple of 16; small_grid: the test hook (it
// caps the table scan's workgroups and changes nothing else).  The summation order picks the template argument, never the kernel.
constexpr Int4ScanPlan int4_scan_plan(int dim, bool codes_aligned16, int64_t n, int compute_units, bool small_grid)
{
    const int64_t tiles = (n + 63) / 64;
    if (dim % 64 != 0 || !codes_aligned16) return {kI4Row, 4, (n + 255) / 256, 0};
    if (dim % 256 == 0 && dim <= kI4TabMaxDim) {
        const int64_t room = (kI4TabLds - static_cast<int64_t>(dim) * 64) / (64 * kI4TabStride);
        const int waves = static_cast<int>(room < kI4TabWaves ? room : kI4TabWaves);
        const int64_t cap = small_grid ? kI4SmallGrid : compute_units > 1 ? compute_units : 1;
        const int64_t want = (tiles + waves - 1) / waves;
        return {kI4Tab, waves, want < cap ? want : cap, static_cast<int64_t>(dim) * 64 + static_cast<int64_t>(waves) * 64 * kI4TabStride};
    }
    return {int4_whole_pieces(dim >> 1) ? kI4Pair128 : kI4PairTail, kI4Waves, (tiles + kI4Waves - 1) / kI4Waves, 0};
}

}  // namespace vg
