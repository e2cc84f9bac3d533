// vg_scan_slices.hpp — into how many slices a whole-segment code scan (SQ8, RaBitQ, PQ ADC) cuts its tiles.  HOST ONLY (no
// HIP): tests/cpp/host_mirror_test.cpp checks it at compile time.
#pragma once

#include <cstdint>

namespace vg {

// `units` workgroups share a slice (queries, or groups of queries that share every code load); tile_groups: how many
// workgroup-iterations of tiles the segment holds.  Enough slices for wg_per_cu workgroups on each of `cus` CUs, a multiple
// of 8 (one group per XCD), at least one iteration of tiles per slice, never fewer than 8.
constexpr int scan_slices(int64_t units, int64_t tile_groups, int cus, int wg_per_cu)
{
    const int64_t want = ((static_cast<int64_t>(wg_per_cu) * cus + units - 1) / units + 7) / 8 * 8;
    const int64_t most = tile_groups / 8 * 8 > 8 ? tile_groups / 8 * 8 : 8;
    return static_cast<int>(want > most ? most : want < 8 ? 8 : want);
}

}  // namespace vg
