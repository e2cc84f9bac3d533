// k_sq8_small.hip — the launcher of the SQ8 nomination's small-batch append GEMM (flat_gemm_sq8_small_kernel,
// vg_sq8_small_gemm.hpp) for gfx950: which 32-query blocks share a launch, its LDS and its persistent grid.  Called by launch_gemm
// (k_flat.hip) for an append over SQ8 code tiles with at most 128 queries.
#include <algorithm>

#include "vg_internal.hpp"
#include "vg_nominate.hpp"
#include "vg_sq8_small_gemm.hpp"

namespace vg {
// Whether one block of 32 queries' image of a dim-dimensional row fits in LDS: the small tile's only limit on dim (dim <= 2528)
bool sq8_small_tile_fits(int dim) { return dim > 0 && sq8_small_lds_bytes(1, (dim + 15) / 16) <= kS8sLdsMax; }

constexpr int kS8sSmallGrid = 2;  // workgroups under the test hook VG_SQ8_SMALL_GRID

// (MASKED, BATCH: a row filter per query / one for the batch — the kernel's variants of their own)
template <bool DOT, int RB, bool MASKED, bool BATCH>
static int32_t launch_rb(size_t lds, int cus, int64_t ntiles, hipStream_t st, const uint16_t *q, int nq, int dim_pad, const uint8_t *tiles, int64_t n,
                         int groups, const float *norms, const float *thr, int thr_stride, int thr_off, int *counts, int count_stride, uint64_t *cand,
                         int cap, const uint8_t *mask, int64_t mask_stride)
{
    auto kern = flat_gemm_sq8_small_kernel<DOT, RB, MASKED, BATCH>;
    VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    // persistent: as many workgroups as the device holds at once (LDS and registers decide how many a CU takes), a tile each at most
    int per_cu = 1;
    VG_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kS8sThreads, lds));
    int64_t grid = std::min<int64_t>(ntiles, static_cast<int64_t>(std::max(cus, 1)) * std::max(per_cu, 1));
    if (hook(kHookSq8SmallGrid)) grid = std::min<int64_t>(grid, kS8sSmallGrid);
    VG_LAUNCH(kern, dim3(static_cast<unsigned>(grid)), dim3(kS8sThreads), lds, st, q, nq, dim_pad, tiles, n, groups, norms, thr, thr_stride, thr_off,
              counts, count_stride, cand, cap, mask, mask_stride);
    return VG_OK;
}

// cnt <= 128 queries (qimg: cnt x dim_pad bfloat16) against the code tiles of n > 0 rows, `groups` 16-dimension groups each.  The
// image of the blocks of a launch is resident in LDS: where all of the batch's blocks do not fit, the batch runs as the fewest
// launches of equally many blocks that do (a pass over the codes each) — decided here, once, from the shapes.
// mask: a device row filter per query (at mask_stride bytes; a launch of the split gets its own queries') or for the batch
// (mask_stride 0: the variant that skips the 64-row code tiles the filter empties, where the filter has the 8 bytes of one — n >= 64 —
// else the per-query variant at stride 0), or null.
template <bool DOT>
int32_t launch_sq8_small_gemm(const uint16_t *qimg, int64_t cnt, int dim_pad, const uint8_t *tiles, int64_t n, int groups, const float *norms,
                              const float *thr, int thr_stride, int thr_off, int *counts, int count_stride, uint64_t *cand, int cap, int cus,
                              hipStream_t st, const uint8_t *mask, int64_t mask_stride)
{
    VG_CHECK(cnt > 0 && cnt <= 128 && n > 0 && groups > 0 && dim_pad >= 32 * sq8_small_steps(groups) && dim_pad % 8 == 0 && aligned16(qimg, tiles) &&
                 sq8_small_lds_bytes(1, groups) <= kS8sLdsMax,
             VG_ERR_INVALID_ARG, "launch_sq8_small_gemm: a call the small SQ8 tile does not take");
    const int rb = static_cast<int>((cnt + 31) / 32);
    int launches = 1;
    while (sq8_small_lds_bytes((rb + launches - 1) / launches, groups) > kS8sLdsMax) launches++;
    const int per = (rb + launches - 1) / launches;  // blocks a launch
    const int64_t ntiles = (n + kS8sBN - 1) / kS8sBN;
    const bool skip = mask && mask_stride == 0 && n >= 64;
    for (int64_t q0 = 0; q0 < cnt; q0 += per * 32) {
        const int qc = static_cast<int>(std::min<int64_t>(per * 32, cnt - q0)), b = (qc + 31) / 32;
        const size_t lds = sq8_small_lds_bytes(b, groups);
        auto go = [&](auto kern_rb) {
            constexpr int RB = decltype(kern_rb)::value;
            auto with = [&](auto masked, auto batch) {
                return launch_rb<DOT, RB, decltype(masked)::value, decltype(batch)::value>(
                    lds, cus, ntiles, st, qimg + q0 * dim_pad, qc, dim_pad, tiles, n, groups, norms, thr + q0 * thr_stride, thr_stride, thr_off,
                    counts + q0 * count_stride, count_stride, cand + q0 * cap, cap, mask ? mask + q0 * mask_stride : nullptr, mask_stride);
            };
            if (!mask) return with(std::false_type{}, std::false_type{});
            return skip ? with(std::true_type{}, std::true_type{}) : with(std::true_type{}, std::false_type{});
        };
        VG_TRY(b == 1   ? go(std::integral_constant<int, 1>{})
               : b == 2 ? go(std::integral_constant<int, 2>{})
               : b == 3 ? go(std::integral_constant<int, 3>{})
                        : go(std::integral_constant<int, 4>{}));
    }
    return VG_OK;
}
template int32_t launch_sq8_small_gemm<false>(const uint16_t *, int64_t, int, const uint8_t *, int64_t, int, const float *, const float *, int, int, int *,
                                              int, uint64_t *, int, int, hipStream_t, const uint8_t *, int64_t);
template int32_t launch_sq8_small_gemm<true>(const uint16_t *, int64_t, int, const uint8_t *, int64_t, int, const float *, const float *, int, int, int *,
                                             int, uint64_t *, int, int, hipStream_t, const uint8_t *, int64_t);
}  // namespace vg
