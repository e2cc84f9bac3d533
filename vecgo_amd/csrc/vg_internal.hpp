// vg_internal.hpp — host-side plumbing shared by the C-ABI translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vecgo_hip.h"

struct vg_index;

#define VG_API extern "C" __attribute__((visibility("default")))

namespace vg {

void set_error(const char *fmt, ...);

#define VG_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::vg::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,   \
                            __LINE__);                                                        \
            (void)hipGetLastError();                                                          \
            return _e == hipErrorOutOfMemory ? VG_ERR_OUT_OF_MEMORY : VG_ERR_HIP;             \
        }                                                                                     \
    } while (0)

// Kernel launch with error check.  HIP keeps a sticky "last error" that some successful calls
// latch (e.g. pointer-attribute probes of plain host memory inside hipMemcpyDefault), so the
// state is cleared right before the launch and read right after it.
#define VG_LAUNCH(...)                                                                              \
    do {                                                                                            \
        (void)hipGetLastError();                                                                    \
        hipLaunchKernelGGL(__VA_ARGS__);                                                            \
        hipError_t _le = hipGetLastError();                                                         \
        if (_le != hipSuccess) {                                                                    \
            ::vg::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_le), __FILE__,   \
                            __LINE__);                                                              \
            return VG_ERR_HIP;                                                                      \
        }                                                                                           \
    } while (0)

#define VG_CHECK(cond, status, ...)          \
    do {                                     \
        if (!(cond)) {                       \
            ::vg::set_error(__VA_ARGS__);    \
            return (status);                 \
        }                                    \
    } while (0)

#define VG_TRY(expr)                   \
    do {                               \
        int32_t _s = (expr);           \
        if (_s != VG_OK) return _s;    \
    } while (0)

bool is_device_ptr(const void *p);

// Test hooks: switches that force a slower or alternative path so the tests can compare the paths.  Read from
// the environment ONCE (first use) and changed afterwards only through vg_debug_set_hook — the entry points
// test one relaxed atomic, never getenv.
enum Hook {
    kHookFlatNoSmallTile,     // VG_FLAT_NO_SMALL_TILE   always the 128-query GEMM tile
    kHookFlatUnfused,         // VG_FLAT_UNFUSED         materialise the score matrix
    kHookFlatNoScan,          // VG_FLAT_NO_SCAN         no small-batch register scan
    kHookFlatForceExact,      // VG_FLAT_FORCE_EXACT     exhaustive exact kernel for every query
    kHookFlatNoDma,           // VG_FLAT_NO_DMA          register-staged GEMM
    kHookFlatDebug,           // VG_FLAT_DEBUG           print per-call counters
    kHookProbeNoGroup,        // VG_PROBE_NO_GROUP       one pass per (query, probe) pair
    kHookAdcBigkExhaustive,   // VG_ADC_BIGK_EXHAUSTIVE  LDS-buffer path for k > 64
    kHookBuildDebug,          // VG_BUILD_DEBUG          vg_hnsw_build prints its back-link totals
    kHookKmNoMfma,            // VG_KM_NO_MFMA           k-means assignment by the reference-order kernels only
    kHookKmListAll,           // VG_KM_LIST_ALL          k-means: the matrix scores decide nothing, every point is listed
    kHookKmBf16,              // VG_KM_BF16              k-means: the bfloat16-split passes even for a single assignment
    kHookKmNoBf16,            // VG_KM_NO_BF16           k-means: fp32 matrix passes only
    kHookBruteNoFlat,         // VG_BRUTE_NO_FLAT        vg_search_hnsw_brute: always the distance matrix + replay
    kHookPqNoMfma,            // VG_PQ_NO_MFMA           PQ Encode / Lloyd assignment by the reference-order kernels only
    kHookPqListAll,           // VG_PQ_LIST_ALL          PQ Encode / assignment: every (row, sub-quantizer) pair is listed
    kHookPqFp32Mfma,          // VG_PQ_FP32_MFMA         PQ Encode / assignment: the fp32 matrix form (pq_nominate_kernel)
    kHookProbeNoGemm,         // VG_PROBE_NO_GEMM        probed fp32 scan: the exact kernels only, no matrix-core nomination
    kHookFlatNoBigTile,       // VG_FLAT_NO_BIG_TILE     bf16 nomination: the 128 x 128 tile even above 128 queries
    kHookFlatBigTile2,        // VG_FLAT_BIG_TILE_2      bf16 256 x 256 tile with two row-tile buffers (128 KiB) instead of three
    kHookFlatBigEarlyB,       // VG_FLAT_BIG_EARLY_B     bf16 256 x 256 tile: row-tile fills behind the first matrix group of a step
    kHookPqNomAlways,         // VG_PQ_NOM_ALWAYS        vg_index_enable_pq_nomination: batches of any size take the nomination
    kHookSq8NomCodesAlways,   // VG_SQ8_NOM_CODES_ALWAYS vg_index_enable_sq8_nomination_from_codes: no crossover of (query, row) pairs
    kHookKmNoRanges,          // VG_KM_NO_RANGES         k-means: the listed points' exact pass in one walk over the centroids (no ranges)
    kHookNoCandReplay,        // VG_NO_CAND_REPLAY       no heap replay for queries whose scores may hold a NaN (vg_cand_replay.hpp): what the fast paths alone answer
    kHookVamanaSmallScratch,  // VG_VAMANA_SMALL_SCRATCH a small batch takes several launches: vg_search_vamana with k > 512 gets 64 MiB of per-launch scratch, the Vamana builders' visited bitmaps (VamanaBatch, vg_vamana_common.hpp) 64 KiB
    kHookFlatRescoreSample,   // VG_FLAT_RESCORE_SAMPLE  flat search: the main GEMM multiplies the sampled row tiles again (no append from the sample)
    kHookPthrForceHist,       // VG_PTHR_FORCE_HIST      vg_search_flat_probed_threshold without rerank: the top-max_results-by-histogram form, then the filter
    kHookWalkSmallScratch,    // VG_WALK_SMALL_SCRATCH   a search walk's batch goes in launches of at most 5 queries (WalkChunks, vg_search.hpp): vg_search_hnsw / _pq / _filtered / _predicate, vg_search_vamana and its kin, vg_search_vamana_fresh
    kHookFlatNoSplit,         // VG_FLAT_NO_SPLIT        vg_search_flat above 128 queries: the fp32 MFMA GEMM, not the split tile (three bf16 products)
    kHookFlatNoScreen,        // VG_FLAT_NO_SCREEN       vg_search_flat on the split tile: no one-product screen in front, the three-product pass for every tile
    kHookFlatScreenFail,      // VG_FLAT_SCREEN_FAIL     vg_search_flat behind a screen: every screen proof counts as failed, every query is retried on the split tile (and the screen runs up to k = 48, not 16)
    kHookFlatF32Sample,       // VG_FLAT_F32_SAMPLE      vg_search_flat on the split tile: the threshold sample stays the fp32 128 x 128 tile's, not the persistent tile's one bf16 product
    kHookPrefilterSmallScratch,  // VG_PREFILTER_SMALL_SCRATCH vg_search_flat_prefilter cuts its query chunks for 64 KiB of lists and keys, not the context's scratch cap: a test batch takes the several chunks a large one takes
    kHookBm25SmallScratch,    // VG_BM25_SMALL_SCRATCH vg_bm25_search cuts its query chunks for 64 KiB of keys, not the context's scratch cap: a test batch takes the several chunks a large one takes
    kHookInt4SmallGrid,       // VG_INT4_SMALL_GRID    vg_int4_l2_distance_batch launches int4_scan_tab_kernel on at most 2 workgroups (vg_int4_plan.hpp), the same kernel, waves and LDS: a few thousand rows give every wave the several tiles it walks over millions
    kHookInt4SearchSmallGrid, // VG_INT4_SEARCH_SMALL_GRID vg_search_int4 launches at most 2 workgroups / 2 slices (the table form through vg_int4_plan.hpp's cap): a few thousand rows give every wave several trips and the merge several lists
    kHookAdcWideAlways,       // VG_ADC_WIDE_ALWAYS    every PQ probed, filtered or threshold scan walks its table in chunks (adc_wide_walk, vg_adc_wide.hpp) whatever m is: the chunk seams at a few rows, wide against narrow results on one index
    kHookRabitqNomAlways,     // VG_RABITQ_NOM_ALWAYS  vg_index_enable_rabitq_nomination: no crossover of (query, row) pairs
    kHookRabitqNomCheck,      // VG_RABITQ_NOM_CHECK   vg_index_enable_rabitq_nomination: the verify compares every listed key's Hamming distance (the GEMM's) with its own popcount and counts the disagreements (vg_index_rabitq_nomination_info's `mismatched`)
    kHookCount
};
bool hook(Hook h);

// Per-call HBM scratch.  Blocks come from a process-wide cache keyed by (device, stream): a block
// released by one call is handed to the next call on the SAME stream, where stream order makes
// the reuse safe without waiting.  (The runtime's own stream-ordered pool, hipMallocAsync, was
// dropped: on ROCm 7.2 / gfx950 a block it recycled after a pool trim came back zero-filled
// after the copy into it had completed — see DESIGN.md "Scratch memory".)
int32_t scratch_alloc(void **out, size_t bytes, hipStream_t s);
// Rows appended to a resident index (vg_hnsw_insert): ||x||^2 and max |x| of rows from .. to-1 of d_vectors
// folded into d_norms / d_norm_max (k_exact.hip); their bfloat16 filter image (k_flat.hip)
int32_t append_row_norms(vg_index *idx, int64_t from, int64_t to, hipStream_t st);
int32_t append_bf16_rows(vg_index *idx, int64_t from, int64_t to, hipStream_t st);
void scratch_free(void *p);
void scratch_trim(int device);

}  // namespace vg

struct vg_prof_record {
    const char *name;
    hipEvent_t start, stop;
};

// Grow-only scratch arena, one per (context, stream): per-call hipMallocAsync of multi-GB
// buffers costs milliseconds of host time; work enqueued on one stream is ordered, so the next
// call on that stream may reuse the same bytes.
struct vg_arena {
    char *base = nullptr;
    size_t cap = 0;
};

struct vg_ctx {
    int device = 0;
    std::mutex arena_mu;
    std::vector<std::pair<hipStream_t, vg_arena>> arenas;
    hipStream_t stream = nullptr;
    int compute_units = 0;
    int64_t hbm_bytes = 0;
    char arch[64] = {0};
    bool profiling = false;
    std::mutex prof_mu;
    std::vector<vg_prof_record> prof;
};

namespace vg {
// RAII bracket around a kernel launch: records an event pair on `st` when profiling is on
struct ProfScope {
    vg_ctx *ctx;
    hipStream_t st;
    vg_prof_record rec{};
    bool active = false;
    ProfScope(vg_ctx *c, const char *name, hipStream_t s) : ctx(c), st(s)
    {
        if (!c->profiling) return;
        // hipEventReleaseToDevice: the event's release is device scope.  A default event makes the kernel in front
        // of it end with a SYSTEM-scope release (L2 write-back walk), which a kernel pays only because it is being
        // timed: measured +6..10 us on a 160 us scan that writes 20 KB (HIP: "useful to obtain more precise
        // timings of commands between events").
        if (hipEventCreateWithFlags(&rec.start, hipEventReleaseToDevice) != hipSuccess) return;
        if (hipEventCreateWithFlags(&rec.stop, hipEventReleaseToDevice) != hipSuccess) {
            (void)hipEventDestroy(rec.start);
            return;
        }
        rec.name = name;
        (void)hipEventRecord(rec.start, st);
        active = true;
    }
    ~ProfScope()
    {
        if (!active) return;
        (void)hipEventRecord(rec.stop, st);
        std::lock_guard<std::mutex> g(ctx->prof_mu);
        ctx->prof.push_back(rec);
    }
};
}  // namespace vg

namespace vg {

inline hipStream_t pick_stream(vg_ctx *ctx, void *stream)
{
    return stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
}

// whether every pointer is 16-byte aligned: the condition of the codecs' and scans' 16-byte loads and stores
template <typename... T>
inline bool aligned16(const T *...p)
{
    return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

// What a call site does with a DEVICE pointer of the caller's that is element-aligned but not 16-byte aligned (a view into
// a larger buffer).  Kernels read and write their operands through wider types (float4, uint4, uint64_t, direct-to-LDS
// loads), so the default hands them a 16-byte aligned copy: the buffer goes through a scratch block by a device-to-device
// copy on the call's stream, outputs come back the same way, and nothing waits.  A call site that tests the pointer itself
// (aligned16) and has a kernel of plain element accesses for the other case says kAnyAlign and keeps the pointer.  A
// 16-byte aligned device pointer is always used where it lies.
enum Align { kStage16, kAnyAlign };
// counts the device buffers staged so: read and cleared by vg_profile_read("staged_device_buffers")
void note_staged_device_buffer();
// launches of the flat search's split tile: read and cleared by vg_profile_read("flat_split_launches")
void note_flat_split_launch();

// Read-only input that may live on the host: staged into HBM for the call.
template <typename T>
struct DevIn {
    const T *ptr = nullptr;
    T *owned = nullptr;
    hipStream_t st = nullptr;
    int32_t init(const T *p, size_t count, hipStream_t s, Align align = kStage16)
    {
        st = s;
        if (count == 0 || p == nullptr) {
            ptr = p;
            return VG_OK;
        }
        const bool dev = is_device_ptr(p);
        if (dev && (align == kAnyAlign || aligned16(p))) {
            ptr = p;
            return VG_OK;
        }
        // Host buffers are the slow path (cgo, tests): staged through a cached HBM block; so is a misaligned device view
        if (dev) note_staged_device_buffer();
        VG_TRY(scratch_alloc(reinterpret_cast<void **>(&owned), count * sizeof(T), s));
        VG_HIP(hipMemcpyAsync(owned, p, count * sizeof(T), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        ptr = owned;
        return VG_OK;
    }
    ~DevIn()
    {
        if (owned) scratch_free(owned);
    }
};

// Output that may live on the host: produced in HBM, copied back by finish().
template <typename T>
struct DevOut {
    T *ptr = nullptr;
    T *owned = nullptr;
    T *host = nullptr;
    T *dev = nullptr;  // a misaligned device buffer of the caller's that `owned` stands in for
    size_t count = 0;
    hipStream_t st = nullptr;
    int32_t init(T *p, size_t n, hipStream_t s, Align align = kStage16)
    {
        st = s;
        count = n;
        if (n == 0 || p == nullptr) {
            ptr = p;
            return VG_OK;
        }
        const bool on_device = is_device_ptr(p);
        if (on_device && (align == kAnyAlign || aligned16(p))) {
            ptr = p;
            return VG_OK;
        }
        (on_device ? dev : host) = p;
        if (on_device) note_staged_device_buffer();
        VG_TRY(scratch_alloc(reinterpret_cast<void **>(&owned), n * sizeof(T), s));
        ptr = owned;
        return VG_OK;
    }
    int32_t finish()
    {
        if (host && count) {
            VG_HIP(hipMemcpyAsync(host, owned, count * sizeof(T), hipMemcpyDeviceToHost, st));
            VG_HIP(hipStreamSynchronize(st));
        }
        if (dev && count) VG_HIP(hipMemcpyAsync(dev, owned, count * sizeof(T), hipMemcpyDeviceToDevice, st));  // stream-ordered: no wait
        return VG_OK;
    }
    ~DevOut()
    {
        if (owned) scratch_free(owned);
    }
};

// Carves 256-byte aligned pieces out of the (context, stream) arena.  Usage: add() every piece,
// then commit() once (grows the arena if needed: synchronises the stream only when it grows),
// then get<T>(i).  The arena mutex is held until the ArenaCall is destroyed, i.e. for the
// duration of the enqueue, which serialises concurrent callers of one (context, stream).
struct ArenaCall {
    vg_ctx *ctx;
    hipStream_t st;
    std::vector<size_t> offs;
    size_t total = 0;
    char *base = nullptr;
    std::unique_lock<std::mutex> lock;
    ArenaCall(vg_ctx *c, hipStream_t s) : ctx(c), st(s), lock(c->arena_mu) {}
    int add(size_t bytes)
    {
        offs.push_back(total);
        total += (bytes + 255) & ~size_t(255);
        return static_cast<int>(offs.size()) - 1;
    }
    int32_t commit()
    {
        vg_arena *a = nullptr;
        for (auto &p : ctx->arenas)
            if (p.first == st) a = &p.second;
        if (!a) {
            ctx->arenas.emplace_back(st, vg_arena{});
            a = &ctx->arenas.back().second;
        }
        if (a->cap < total) {
            if (a->base) {
                VG_HIP(hipStreamSynchronize(st));
                VG_HIP(hipFree(a->base));
                a->base = nullptr;
                a->cap = 0;
            }
            size_t want = total + total / 4;
            VG_HIP(hipMalloc(reinterpret_cast<void **>(&a->base), want));
            a->cap = want;
        }
        base = a->base;
        return VG_OK;
    }
    template <typename T>
    T *get(int i) const
    {
        return reinterpret_cast<T *>(base + offs[static_cast<size_t>(i)]);
    }
};

// One piece of a call's scratch after the other, each 256-byte aligned; base null: only the sizes are added up
struct Carve {
    char *base;
    size_t off = 0;
    template <typename T>
    void take(T *&p, int64_t count)
    {
        p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += (static_cast<size_t>(count) * sizeof(T) + 255) & ~size_t(255);
    }
};

// Scratch in HBM for the duration of a call (cached block, see scratch_alloc).
template <typename T>
struct DevTmp {
    T *ptr = nullptr;
    hipStream_t st = nullptr;
    int32_t init(size_t count, hipStream_t s)
    {
        st = s;
        if (count == 0) return VG_OK;
        VG_TRY(scratch_alloc(reinterpret_cast<void **>(&ptr), count * sizeof(T), s));
        return VG_OK;
    }
    ~DevTmp()
    {
        if (ptr) scratch_free(ptr);
    }
};

// A device array of the call's own (hipMalloc, at least one element): freed at return unless release() hands it on
template <typename T>
struct DevBuf {
    T *p = nullptr;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    int32_t alloc(size_t count)
    {
        VG_HIP(hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(count, 1) * sizeof(T)));
        return VG_OK;
    }
    T *release()
    {
        T *r = p;
        p = nullptr;
        return r;
    }
};

// Frees the device array a slot holds, if any, and leaves the slot null.  Work that may still read the array is the
// caller's to wait for.
template <typename T>
inline void drop_device(T **slot)
{
    if (*slot) (void)hipFree(*slot);
    *slot = nullptr;
}

// The grid of a row-walk codec kernel (sq8_encode4_kernel, k_sq8.hip): a thread owns a few consecutive dimensions and walks
// rpt rows, blocks_y = gridDim.y covers the n rows.
constexpr int kRowsPerThread = 16;  // at least; more when n / 16 exceeds the grid's y range
inline int rows_per_thread(int64_t n) { return static_cast<int>(std::max<int64_t>(kRowsPerThread, (n + 65534) / 65535)); }
struct RowWalk {
    int rpt;
    unsigned blocks_y;
    explicit RowWalk(int64_t n) : rpt(rows_per_thread(n)), blocks_y(static_cast<unsigned>((n + rpt - 1) / rpt)) {}
};

}  // namespace vg

struct vg_pq {
    vg_ctx *ctx = nullptr;
    int32_t dim = 0, m = 0, k = 0, subdim = 0;
    bool trained = false;
    int8_t *d_codebooks = nullptr;  // m*k*subdim
    float *d_scales = nullptr;      // m
    float *d_offsets = nullptr;     // m
};

namespace vg {
// What vg_pq_train refuses about a quantizer's shape and n training rows, with its status and message: for the builders
// (vg_flat_build, vg_diskann_build), which refuse before they change anything.
inline int32_t pq_train_refusal(const vg_pq *pq, int64_t n)
{
    VG_CHECK(n <= INT32_MAX, VG_ERR_UNSUPPORTED, "vg_pq_train: more than 2^31-1 training vectors");
    VG_CHECK(pq->subdim <= 256, VG_ERR_UNSUPPORTED, "vg_pq_train: sub-vector dim %d > 256", pq->subdim);
    VG_CHECK(static_cast<size_t>(pq->k) * pq->subdim * sizeof(float) <= 152 * 1024, VG_ERR_UNSUPPORTED,
             "vg_pq_train: codebook of one sub-quantizer exceeds 152 KiB");
    return VG_OK;
}
}  // namespace vg

struct vg_sq8 {
    vg_ctx *ctx = nullptr;
    int32_t dim = 0;
    bool trained = false;
    float *d_mins = nullptr, *d_maxs = nullptr, *d_scales = nullptr, *d_inv = nullptr;  // [dim] each, one block: mins, maxs, scales, inverse scales
};

struct vg_int4 {
    vg_ctx *ctx = nullptr;
    int32_t dim = 0;
    bool trained = false;
    float *d_min = nullptr, *d_diff = nullptr;  // [dim] each
    float *d_table = nullptr;                   // [dim * 16] BuildInt4LookupTable
};

namespace vg {
// Partition-probed scans (k_probe.hip): (query, probe) pairs bucketed by partition and cut into groups
// of up to kProbeQB pairs; one workgroup scores a slice of the partition's rows against a whole group.
constexpr int kProbeQB = 8;
struct ProbeGroup {
    uint32_t part;   // partition
    uint32_t first;  // first entry of the group in pair_of[]
    uint32_t count;  // 1..kProbeQB
};
// The grouped nomination of the probed scans (flat_probe_gemm, k_flat.hip), where the caller re-scores with its own exact
// distance (SQ8: launch_sq8_verify, k_sq8_scan.hip): per (query, probe) pair its thresholds, how many rows fell below the last one,
// and those rows.
struct ProbeNominated {
    float *thr;            // [pairs, sel_k]: the pair's threshold is entry sel_k - 1
    int *counts;           // [pairs]
    uint32_t *cand_id;     // [pairs, 64]: the 64 best appended rows ascending by nomination score (k <= 48 only)
    float *cand_sc;
    int cap;               // appended keys kept per pair (counts above it: rows were dropped)
    int sel_k;
    uint64_t *cand;        // [pairs, cap]: every appended key (k > 48: all of them are re-scored)
};
constexpr int kProbeGemmMaxK = 160;  // deepest threshold: the 60th best of the 1/8 row sample, ~480 rows pass it
// A bfloat16 row image the matrix-core nomination runs on (vg_nominate.hpp): a quantizer's DECODED rows rounded to bfloat16
// (vg_index_enable_sq8_nomination, vg_index_enable_pq_nomination; all null when off), or a view of the fp32 rows' bf16 filter.
// The PQ nomination FROM THE CODES (vg_index_enable_pq_nomination_from_codes, k_pq_nominate.hip) keeps no decoded-row image: the
// nomination GEMM's row tile is gathered from a bfloat16 copy of the decoded codebook, granule by granule (sub-dimension 8: a
// 16-byte granule of a decoded row IS one centroid).  Its state is the same object with that codebook in the rows' place
// (from_codes), so an index holds one PQ nomination or the other, never both.
struct NomImage {
    uint16_t *rows = nullptr;  // n * dim_pad; from_codes: [dim_pad / 8][256][8], entry (j, c) = centroid c of sub-quantizer j decoded and rounded; j >= m: zeros
    int32_t dim_pad = 0;       // the row length: dim padded with zeros to whole 64-element K steps of the bf16 GEMM
    float *norms = nullptr;    // n: |x^|^2 (fp32 of the unrounded values)
    float *norm_max = nullptr; // [1]: the largest of them
    bool from_codes = false;   // `rows` is the decoded codebook, not the decoded rows
    // The SQ8 nomination from the codes (vg_index_enable_sq8_nomination_from_codes, k_sq8_scan.hip): from_codes with `scale` set.
    // `rows` holds dim_pad floats, mid_d = min_d + 128 inv_d (zeros from dim on) — the offset of its score space; the GEMM's row
    // tile is converted from the code tiles, bf16(code - 128), and the queries are multiplied by `scale` before they are rounded.
    const float *scale = nullptr;  // the quantizer's inverse scales (borrowed), or null
    int64_t body = 0;              // bytes of `rows`
    // what vg_index_pq_nomination_info reports: 0 off, 1 the image of the decoded rows, 2 from the codes
    int mode() const { return !rows ? 0 : from_codes ? 2 : 1; }
    uint16_t *row_image() const { return from_codes ? nullptr : rows; }  // the decoded rows, where the mode keeps them
    static int64_t body_bytes(int64_t n, int dim_pad, bool from_codes) { return (from_codes ? int64_t(dim_pad / 8) * 256 * 8 : n * dim_pad) * 2; }
    int64_t held_bytes(int64_t n) const { return rows ? body + n * 4 + 4 : 0; }  // the body, the norms, norm_max
};
// Frees an image (after the stream's work that may read it) and leaves it empty.
inline int32_t nom_free(NomImage &img, hipStream_t st)
{
    if (!img.rows) return VG_OK;
    VG_HIP(hipStreamSynchronize(st));
    VG_HIP(hipFree(img.rows));
    VG_HIP(hipFree(img.norms));
    VG_HIP(hipFree(img.norm_max));
    img = NomImage{};
    return VG_OK;
}
}  // namespace vg

struct vg_index {
    vg_ctx *ctx = nullptr;
    int64_t n = 0;
    int32_t dim = 0;
    int32_t metric = 0;
    // PQ codes, re-tiled: [tile][group][lane][16 B]; see k_adc.hip
    vg_pq *pq = nullptr;
    uint8_t *d_pq_tiles = nullptr;
    int64_t n_tiles = 0;
    int32_t pq_groups = 0;  // ceil(m/16)
    // fp32 rows, row-major n*dim (reference layout), plus ||x||^2 for the GEMM path
    float *d_vectors = nullptr;
    float *d_norms = nullptr;
    float *d_norm_max = nullptr;  // [1] max ||x||^2: error bound of the GEMM-form scores
    uint16_t *d_vectors_bf16 = nullptr;  // optional bfloat16 copy of the rows: vg_index_enable_bf16_filter
    int32_t vectors_bf16_dim = 0;        // its row length: dim padded with zeros to whole 64-element K steps of the bf16 GEMM
    unsigned long long *d_flat_stats = nullptr;  // [4] queries searched, queries sent to the exhaustive kernel, queries retried on the split tile behind a screen, candidates the fused path appended (vg_index_flat_appended)
    // RaBitQ: sign bits re-tiled [tile][group][lane][16 B] and the stored norms
    uint8_t *d_rq_tiles = nullptr;
    float *d_rq_norms = nullptr;
    int32_t rq_groups = 0;  // ceil(((dim+63)/64*8) / 16)
    // vg_index_enable_rabitq_nomination (k_rabitq_nominate.hip): nothing resident — the mode's GEMM reads the tiles and norms above
    bool rq_nom_on = false;
    bool rq_nom_negative = false;    // a stored norm is negative: the screen's inequality does not hold, every batch keeps the scan
    int64_t rq_nom_rescanned = 0;    // queries whose proof failed and the scan answered, since the mode was enabled
    int64_t rq_nom_mismatched = 0;   // VG_RABITQ_NOM_CHECK: listed keys whose Hamming distance was not the popcount's
    // HNSW adjacency
    uint32_t *d_hnsw_l0 = nullptr;     // n*m0
    float *d_hnsw_l0_dist = nullptr;   // n*m0 cached edge distances (Neighbor.Dist) for the predicate-aware walk, or null
    // the distances a GPU-built graph cached per slot as its inserts computed them (layer 0: like d_hnsw_l0, upper levels:
    // like d_hnsw_adj), kept by vg_hnsw_build / vg_hnsw_insert for the next vg_hnsw_insert; null for an uploaded graph
    float *d_hnsw_l0_cdist = nullptr, *d_hnsw_adj_cdist = nullptr;
    uint8_t *d_hnsw_tomb = nullptr;    // g.tombstones as a bitmap (ceil(n/8) bytes), or null: no deleted node
    uint32_t *d_hnsw_slot = nullptr;   // max_level*n
    uint32_t *d_hnsw_adj = nullptr;    // concatenated level tables
    int64_t *d_hnsw_level_off = nullptr;  // max_level+1 row offsets into d_hnsw_adj (in rows)
    int32_t hnsw_m0 = 0, hnsw_m = 0, hnsw_max_level = 0;
    uint32_t hnsw_entry = 0;
    // rows that d_vectors / d_norms, d_vectors_bf16, d_hnsw_l0 and d_hnsw_tomb have room for: vg_hnsw_insert grows
    // them by capacity; 0 = exactly n (every other entry point allocates them at n and resets these)
    int64_t rows_cap = 0, bf16_cap = 0, l0_cap = 0, tomb_cap = 0;
    // Vamana adjacency
    uint32_t *d_vamana = nullptr;      // n*r
    int64_t vamana_cap = 0;            // rows d_vamana has room for: vg_vamana_insert grows it by capacity; 0 = exactly n
    int32_t vamana_r = 0;
    uint32_t vamana_entry = 0;
    // PQ codes in the reference's row-major layout (random access by node id in graph search)
    uint8_t *d_pq_rows = nullptr;
    vg::NomImage pq_nom;               // vg_index_enable_pq_nomination: the DECODED rows (pq.go:185-229); _from_codes: the decoded CODEBOOK
    uint8_t *d_rq_rows = nullptr;
    // SQ8 codes, re-tiled like the PQ codes: [tile][group of 16 dims][lane][16 B]; see k_sq8_scan.hip
    vg_sq8 *sq = nullptr;
    vg::NomImage sq_nom;               // vg_index_enable_sq8_nomination: the dequantised codes; _from_codes: the score space's offset
    int64_t sq_nom_rescanned = 0;      // queries whose proof failed and the scan answered, since sq_nom was enabled
    uint8_t *d_sq_tiles = nullptr;
    int32_t sq_groups = 0;  // ceil(dim/16)
    // INT4 codes of a DiskANN segment, row-major n * ceil(dim/2), and the quantizer's lookup table
    uint8_t *d_int4_rows = nullptr;
    const float *int4_table = nullptr;  // borrowed from the vg_int4
    const float *int4_min = nullptr, *int4_diff = nullptr;  // (same)
    // IVF partitions of a flat segment: centroids [P*dim], first row of every partition [P+1]
    float *d_centroids = nullptr;
    uint32_t *d_part_off = nullptr;
    std::vector<uint32_t> h_part_off;  // the same on the host (launch bounds of the grouped GEMM, k_probe.hip)
    int32_t num_partitions = 0;
};

namespace vg {
// What a segment's index holds besides fp32 rows and an HNSW graph, or null: rows appended or lists rewritten by a
// memtable's entry point (vg_hnsw_insert, vg_hnsw_compact) would leave it behind
// (a PQ nomination, pq_nom, has no arm: it exists only beside d_pq_rows — both enable functions want the codes, and
// vg_index_set_pq_codes frees it before it replaces them — so "PQ codes" answers for it)
inline const char *held_segment_state(const vg_index *idx)
{
    return (idx->d_pq_tiles || idx->d_pq_rows)   ? "PQ codes"
           : idx->d_sq_tiles                     ? "SQ8 codes"
           : idx->d_int4_rows                    ? "INT4 codes"
           : (idx->d_rq_tiles || idx->d_rq_rows) ? "RaBitQ codes"
           : idx->d_centroids                    ? "IVF partitions"
           : idx->d_vamana                       ? "a Vamana graph"
           : idx->sq_nom.rows                    ? "an SQ8 nomination image"
                                                 : nullptr;
}
// The same for the streaming Vamana insert (vg_vamana_insert): what its new rows would lack, or null
inline const char *held_fresh_state(const vg_index *idx)
{
    return (idx->d_pq_tiles || idx->d_pq_rows)   ? "PQ codes"
           : idx->d_sq_tiles                     ? "SQ8 codes"
           : idx->d_int4_rows                    ? "INT4 codes"
           : (idx->d_rq_tiles || idx->d_rq_rows) ? "RaBitQ codes"
           : idx->d_centroids                    ? "IVF partitions"
           : idx->d_hnsw_l0                      ? "an HNSW graph"
           : idx->d_hnsw_tomb                    ? "HNSW tombstones"
           : idx->sq_nom.rows                    ? "an SQ8 nomination image"
                                                 : nullptr;
}
}  // namespace vg
