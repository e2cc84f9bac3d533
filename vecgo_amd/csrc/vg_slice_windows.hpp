// vg_slice_windows.hpp — a batch row filter as one wave of a small append tile reads it (flat_gemm_pq_small_kernel<RB, true, true>,
// vg_pq_small_gemm.hpp; flat_gemm_sq8_small_kernel<DOT, RB, true, true>, vg_sq8_small_gemm.hpp).  Both tiles have the same geometry:
// 256 threads as four waves, a row tile of kSliceBN = 256 rows, wave w owning rows 64 w .. 64 w + 63 of it — 8 bytes of the filter, a
// SLICE — and workgroups persistent over the row tiles (blockIdx.x, + gridDim.x, ...).  A wave skips the tiles whose slice is zero.
// The wave's tiles by ordinal i (tile first + i G, i < mine), the wave's 8 filter bytes of 64 of them a WINDOW, one tile a lane,
// kept as a wave-uniform bitmap of the slices that keep a row: one load instruction whatever the length, so the longest window a
// ballot holds.  The next window is loaded WHEN THE CURRENT ONE IS SPENT and waited for there — why not a window ahead: the note on
// row filters in vg_pq_small_gemm.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vg {

constexpr int kSliceBN = 256, kSliceWindow = 64;
struct SliceNoFilter {};  // what a variant without the skip holds in the windows' place
struct SliceFilterWindows {
    const uint8_t *mask;
    int64_t mask_bytes;  // (n + 7) / 8 >= 8: the launch's condition for these variants
    int first, G, wave, lane, mine;
    uint64_t live;  // bit l: ordinal kSliceWindow win_at + l keeps a row (wave-uniform; clear from `mine` on)
    int win_at;
    // lane l: where the 8 filter bytes of this wave's rows in the tile of ordinal kSliceWindow w + l start
    __device__ __forceinline__ int64_t slice_at(int w) const
    {
        return (first + (static_cast<int64_t>(kSliceWindow) * w + lane) * G) * (kSliceBN / 8) + wave * 8;
    }
    // ... the load of them: unconditional, 8 bytes at any alignment, and never outside the filter — a slice that ends past it (the
    // last tile's, or an ordinal that is no tile) reads the filter's last 8 bytes
    __device__ __forceinline__ uint64_t load_window(int w) const
    {
        const int64_t at = slice_at(w), last = mask_bytes - 8;
        uint64_t v;
        __builtin_memcpy(&v, mask + (at > last ? last : at), 8);
        return v;
    }
    // ... and the slice's 64 bits from what was loaded: shifted down where the address was clamped, zeros coming in; zeros for an
    // ordinal from `mine` on
    __device__ __forceinline__ uint64_t window_bits(int w, uint64_t v) const
    {
        const int64_t at = slice_at(w), last = mask_bytes - 8, over = at > last ? at - last : 0;
        v = over >= 8 ? 0 : v >> (8 * over);
        return static_cast<int64_t>(kSliceWindow) * w + lane < mine ? v : 0;
    }
    // the next window becomes the current one: loaded and waited for here, the one place where the stream drains for the filter
    __device__ __forceinline__ void enter()
    {
        win_at++;
        live = __ballot(window_bits(win_at, load_window(win_at)) != 0);
    }
    // the first ordinal >= i (in window win_at or behind it; i <= the window's end + 1) whose slice keeps a row; `mine`: none
    __device__ __forceinline__ int next_live(int i)
    {
        if (i >= mine) return mine;
        if (i / kSliceWindow == win_at) {
            const uint64_t m = live & (~uint64_t(0) << (i % kSliceWindow));
            if (m != 0) return win_at * kSliceWindow + __builtin_ctzll(m);
        }
        do {  // the windows behind it, until one keeps a row
            if ((win_at + 1) * kSliceWindow >= mine) return mine;
            enter();
        } while (live == 0);
        return win_at * kSliceWindow + __builtin_ctzll(live);
    }
    // window 0 loaded; the wave's first live ordinal
    __device__ __forceinline__ int init(const uint8_t *mask_, int64_t n, int ntiles, int G_, int wave_, int lane_)
    {
        mask = mask_, mask_bytes = (n + 7) >> 3, first = static_cast<int>(blockIdx.x), G = G_, wave = wave_, lane = lane_;
        mine = (ntiles - first + G - 1) / G;
        win_at = -1;
        enter();
        return next_live(0);
    }
};

}  // namespace vg
