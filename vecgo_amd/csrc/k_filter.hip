// k_filter.hip — metadata filters evaluated on the device: resident columns -> one row mask (and match count) per query.
//
//   vg_columns_*        the metadata columns of one segment, resident: per field 0..63 either one f64 per row with a
//                       presence bitmap (numeric fields; ints as float64(I64), numeric_index.go:1072-1076) or one uint32
//                       dictionary code per row (categorical fields; VG_INVALID_ID = the row has no value; the reference
//                       keeps one bitmap per (key, value), unified.go:316-348, getBitmapLocked :1614).
//   vg_filter_evaluate  UnifiedIndex.EvaluateFilter (internal/metadata/unified.go:279-416) for a batch of filter sets.
//   vg_mask_combine     simd.AndWords / AndNotWords / OrWords / XorWords (internal/simd/bitmap.go:26-48) per query.
//   vg_mask_popcount    simd.PopcountWords (bitmap.go:50-55), bits below `rows` only.
//
// Semantics (the reference's): a filter set is the AND of its filters; an empty set matches every row (unified.go:280-282);
// a filter on a field the segment has no column for matches nothing (numeric_index.go:1065-1068, unified.go:318-321).  A
// numeric row matches iff it HAS a value and compareFloat64(value, op, filterVal) holds (numeric_index.go:1020-1037, what
// MatchRowID uses): rows without the field never match, `ne` included (:1176-1182, :1211-1228).  The reference's range
// path with math.Nextafter (:488-497) equals the strict compare for every non-NaN value.  For a stored NaN under `ne` the
// reference's own paths disagree (the bitmap path and compareFloat64 keep the row, the sorted column scan drops it): THIS
// LIBRARY FOLLOWS compareFloat64, a stated choice — the compares below are IEEE compares, so a NaN filter value matches
// nothing except under `ne`, where it matches every present row.  Codes: `eq` matches the rows whose code is the clause's,
// `in` those whose code is in the clause's set; an empty set matches nothing (unified.go:327-330).
//
// The kernel.  A workgroup owns a tile of kFilterTile = 4096 rows and a chunk of the queries; it stages the tile's slice
// of the first kFilterSlots columns its queries reference in LDS once (columns beyond them are read from L2 where they
// lie) and then loops over its queries, one wave per query.  A wave holds 64 consecutive rows, so the 64-bit ballot of a
// clause's compare over row group g IS the mask word of those rows: no bit is packed.  The ballots of the tile's 64 groups
// are collected one per lane (v_writelane: lane g keeps group g's word), so the clause's op is decided once per 4096
// rows — the inner loop is half a 16-byte LDS read, ONE v_cmp_*_f64 against a wave-uniform constant and two lane writes — and the
// presence word, the deleted word and the AND over the clauses are plain 64-bit lane operations.  The finished words
// leave in one store instruction per (query, tile): 512 contiguous bytes.  Counts are integer popcounts of the stored
// words, added atomically per (query, tile): deterministic.  An `in` set is staged in LDS, sorted there by the wave
// (bitonic, padded with 0xFFFFFFFF) and bisected: 12 LDS reads per row at the 4096-code limit, which is also what keeps a
// set to 16 KiB.
#include "vg_device.hpp"
#include "vg_internal.hpp"

struct vg_columns {
    vg_ctx *ctx = nullptr;
    int64_t rows = 0;
    int64_t tiles = 0;  // every array below is allocated and zero-filled to whole tiles
    struct Col {
        int kind = 0;                 // 0 none, 1 f64, 2 codes
        void *data = nullptr;         // tiles * kFilterTile values
        uint64_t *present = nullptr;  // tiles * 64 words, or null: every row has a value
    } col[64];
};

namespace vg {
namespace {

constexpr int kFilterTile = VG_FILTER_TILE_ROWS;  // rows of one workgroup: 64 groups of 64 rows
constexpr int kFilterWaves = 4;                   // each takes every fourth query of the workgroup's chunk
constexpr int kFilterThreads = kFilterWaves * kWave;
constexpr int kFilterSlots = 2;                   // columns staged in LDS per workgroup (32 KiB each)
constexpr int kFilterMaxClauses = 16;
constexpr int kFilterMaxSet = 4096;
constexpr int kFilterStageQueries = 256;          // queries of a chunk whose offsets, and
constexpr int kFilterStageClauses = 640;          // clauses of a chunk that are staged in LDS (the rest are read where they lie)
constexpr int kColNone = 0, kColF64 = 1, kColCodes = 2;
static_assert(kFilterTile == 64 * kWave, "a lane keeps one 64-row word of the tile");

struct FilterCols {
    const void *data[64];
    const uint64_t *present[64];
    uint8_t kind[64];
};

// v_writelane_b32: lane `lane` of `old` <- the wave-uniform `value` (clang has no builtin of that name; the compiler knows
// the intrinsic and pads its hazards)
extern "C" __device__ int vg_llvm_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ uint32_t write_lane(uint32_t value, int lane, uint32_t old)
{
    return static_cast<uint32_t>(vg_llvm_writelane(static_cast<int>(value), lane, static_cast<int>(old)));
}

// the sum of c over the wave, wave-uniform: four DPP steps give every lane its 16-lane row's sum (no LDS round trips, which
// a wave alone on its SIMD cannot hide), four lane reads add the rows
__device__ __forceinline__ int wave_sum(int c)
{
    c += __builtin_amdgcn_update_dpp(0, c, 0xB1, 0xF, 0xF, false);   // quad_perm [1, 0, 3, 2]
    c += __builtin_amdgcn_update_dpp(0, c, 0x4E, 0xF, 0xF, false);   // quad_perm [2, 3, 0, 1]
    c += __builtin_amdgcn_update_dpp(0, c, 0x141, 0xF, 0xF, false);  // row_half_mirror
    c += __builtin_amdgcn_update_dpp(0, c, 0x140, 0xF, 0xF, false);  // row_mirror
    return __builtin_amdgcn_readlane(c, 0) + __builtin_amdgcn_readlane(c, 16) + __builtin_amdgcn_readlane(c, 32) +
           __builtin_amdgcn_readlane(c, 48);
}

__device__ __forceinline__ int uniform_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uniform_f64(double v)
{
    const uint64_t u = static_cast<uint64_t>(__double_as_longlong(v));
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(u));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(u >> 32));
    return __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(hi) << 32) | lo));
}

// lane g <- the ballot of pred over the tile's row group g (rows g * 64 .. g * 64 + 63 of src)
template <typename T, typename Pred>
__device__ __forceinline__ uint64_t filter_sweep(const T *src, int lane, Pred pred)
{
    uint32_t lo = 0, hi = 0;
#pragma unroll 8
    for (int g = 0; g < 64; g++) {
        const uint64_t b = __ballot(pred(src[g * kWave + lane]));
        lo = write_lane(static_cast<uint32_t>(b), g, lo);
        hi = write_lane(static_cast<uint32_t>(b >> 32), g, hi);
    }
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// The same over a column slice staged in LDS as pairs: element (p * 64 + lane) holds the lane's values of row groups 2p and
// 2p + 1, so one 16-byte LDS read (the full 256 B per clock) feeds two compares.  Fully unrolled: the lane numbers are
// constants and all of a sweep's reads are in flight before the first compare.
typedef double filter_f2v __attribute__((ext_vector_type(2)));
template <typename Pred>
__device__ __forceinline__ uint64_t filter_sweep_pairs(const filter_f2v *src, int lane, Pred pred)
{
    filter_f2v v[32];  // (128 VGPRs: the kernel runs one wave per SIMD, its LDS decides that)
#pragma unroll
    for (int p = 0; p < 32; p++) v[p] = src[p * kWave + lane];
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int p = 0; p < 32; p++) {
        const uint64_t b0 = __ballot(pred(v[p].x)), b1 = __ballot(pred(v[p].y));
        lo = write_lane(static_cast<uint32_t>(b0), 2 * p, lo);
        hi = write_lane(static_cast<uint32_t>(b0 >> 32), 2 * p, hi);
        lo = write_lane(static_cast<uint32_t>(b1), 2 * p + 1, lo);
        hi = write_lane(static_cast<uint32_t>(b1 >> 32), 2 * p + 1, hi);
    }
    return (static_cast<uint64_t>(hi) << 32) | lo;
}
// where row r of the tile sits in a slot staged as pairs
__device__ __forceinline__ int filter_pair_index(int r) { return ((((r >> 7) * kWave) + (r & 63)) << 1) | ((r >> 6) & 1); }

// PAIRS: src is an LDS slot staged as pairs; otherwise the column where it lies (row order)
template <bool PAIRS>
__device__ __forceinline__ uint64_t filter_sweep_f64(const double *src, int lane, int op, double c)
{
#define VG_FILTER_SWEEP(CMP)                                                                                                      \
    (PAIRS ? filter_sweep_pairs(reinterpret_cast<const filter_f2v *>(src), lane, [c](double v) { return v CMP c; })               \
           : filter_sweep(src, lane, [c](double v) { return v CMP c; }))
    switch (op) {
        case VG_FILTER_EQ: return VG_FILTER_SWEEP(==);
        case VG_FILTER_NE: return VG_FILTER_SWEEP(!=);
        case VG_FILTER_LT: return VG_FILTER_SWEEP(<);
        case VG_FILTER_LTE: return VG_FILTER_SWEEP(<=);
        case VG_FILTER_GT: return VG_FILTER_SWEEP(>);
        case VG_FILTER_GTE: return VG_FILTER_SWEEP(>=);
        default: return 0;
    }
#undef VG_FILTER_SWEEP
}

// the wave's own sort of n (a power of two) codes in LDS; no workgroup barrier: the waves are at different queries
__device__ __forceinline__ void filter_wave_sort(uint32_t *buf, int n, int lane)
{
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (n >> 1); t += kWave) {
                const int lo = 2 * t - (t & (stride - 1));  // (t / stride) * 2 * stride + t % stride, stride a power of two
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint32_t a = buf[lo], b = buf[hi];
                if ((a > b) == up) {
                    buf[lo] = b;
                    buf[hi] = a;
                }
            }
            __threadfence_block();  // a wave's LDS accesses complete in order; this keeps the compiler's order too
        }
    }
}

// whether `code` is among the n2 (a power of two, >= 1) ascending codes
__device__ __forceinline__ bool filter_in_set(const uint32_t *set, int n2, uint32_t code)
{
    int pos = 0;
    for (int step = n2 >> 1; step > 0; step >>= 1)
        if (set[pos + step - 1] < code) pos += step;
    return set[pos] == code;
}

__global__ __launch_bounds__(kFilterThreads) void filter_eval_kernel(FilterCols cols, const vg_filter_clause *__restrict__ clauses,
                                                                     const int32_t *__restrict__ clause_off, int64_t nq, int q_chunk,
                                                                     const uint32_t *__restrict__ sets, int64_t n_sets,
                                                                     const uint64_t *__restrict__ deleted, int64_t rows,
                                                                     uint8_t *__restrict__ mask, int64_t mask_stride, int word_stores,
                                                                     unsigned long long *__restrict__ counts)
{
    __shared__ __attribute__((aligned(16))) uint64_t slot_mem[kFilterSlots][kFilterTile];  // f64 slices as pairs (filter_sweep_pairs), codes in row order
    __shared__ uint32_t set_mem[kFilterWaves][kFilterMaxSet];
    __shared__ unsigned long long used_fields;
    __shared__ vg_filter_clause cl_mem[kFilterStageClauses];  // a wave alone on its SIMD has nothing to hide a dependent global read behind
    __shared__ int off_mem[kFilterStageQueries + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t q_begin = static_cast<int64_t>(blockIdx.y) * q_chunk;
    const int64_t q_end = q_begin + q_chunk < nq ? q_begin + q_chunk : nq;
    const int64_t word = tile * 64 + lane;  // the mask word this lane keeps
    const int64_t nbytes = (rows + 7) >> 3;

    // rows of this lane's word that exist, less the deleted ones
    const int64_t left = rows - word * 64;
    uint64_t base = left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1 : 0ull;
    if (deleted) base &= ~deleted[word];

    // the columns this chunk's clauses name; the first kFilterSlots of them that exist are staged
    if (tid == 0) used_fields = 0ull;
    __syncthreads();
    const int c_begin = clause_off[q_begin], c_end = clause_off[q_end];
    for (int64_t i = tid; i <= q_end - q_begin && i <= kFilterStageQueries; i += kFilterThreads) off_mem[i] = clause_off[q_begin + i];
    for (int i = tid; i < c_end - c_begin && i < kFilterStageClauses; i += kFilterThreads) cl_mem[i] = clauses[c_begin + i];
    {
        unsigned long long used = 0ull;
        for (int i = c_begin + tid; i < c_end; i += kFilterThreads) {
            const int f = clauses[i].field;
            if (f >= 0 && f < 64 && cols.kind[f] != kColNone) used |= 1ull << f;
        }
        if (used) atomicOr(&used_fields, used);
    }
    __syncthreads();
    int slot_field[kFilterSlots];
    {
        unsigned long long used = used_fields;
#pragma unroll
        for (int s = 0; s < kFilterSlots; s++) {
            slot_field[s] = uniform_i32(used ? __builtin_ctzll(used) : -1);
            if (used) used &= used - 1;
        }
    }
    uint64_t slot_present[kFilterSlots];
#pragma unroll
    for (int s = 0; s < kFilterSlots; s++) {
        slot_present[s] = ~0ull;
        const int f = slot_field[s];
        if (f < 0) continue;
        if (cols.kind[f] == kColF64) {
            const uint64_t *src = static_cast<const uint64_t *>(cols.data[f]) + tile * kFilterTile;
            for (int i = tid; i < kFilterTile; i += kFilterThreads) slot_mem[s][filter_pair_index(i)] = src[i];
        } else {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(static_cast<const uint32_t *>(cols.data[f]) + tile * kFilterTile);
            for (int i = tid; i < kFilterTile / 2; i += kFilterThreads) slot_mem[s][i] = src[i];
        }
        if (cols.present[f]) slot_present[s] = cols.present[f][word];
    }
    __syncthreads();

    uint32_t *my_set = set_mem[wave];
    for (int64_t q = q_begin + wave; q < q_end; q += kFilterWaves) {
        const bool off_staged = q + 1 - q_begin <= kFilterStageQueries;
        const int cb = uniform_i32(off_staged ? off_mem[q - q_begin] : clause_off[q]);
        int nc = uniform_i32(off_staged ? off_mem[q + 1 - q_begin] : clause_off[q + 1]) - cb;
        nc = nc < 0 ? 0 : nc > kFilterMaxClauses ? kFilterMaxClauses : nc;  // (the host has refused both where it can read them)
        uint64_t acc = base;
        for (int ci = cb; ci < cb + nc; ci++) {
            const vg_filter_clause cl = (ci >= c_begin && ci - c_begin < kFilterStageClauses) ? cl_mem[ci - c_begin] : clauses[ci];
            const int f = uniform_i32(cl.field), op = uniform_i32(cl.op);
            const int kind = (f >= 0 && f < 64) ? cols.kind[f] : kColNone;
            if (kind == kColNone) {  // no such column: the filter matches nothing
                acc = 0ull;
                break;
            }
            int slot = -1;
            uint64_t present = ~0ull;
#pragma unroll
            for (int s = 0; s < kFilterSlots; s++)
                if (f == slot_field[s]) {
                    slot = s;
                    present = slot_present[s];
                }
            if (slot < 0 && cols.present[f]) present = cols.present[f][word];
            uint64_t w = 0ull;
            if (kind == kColF64) {
                const double c = uniform_f64(cl.value);
                if (slot == 0)
                    w = filter_sweep_f64<true>(reinterpret_cast<const double *>(slot_mem[0]), lane, op, c);
                else if (slot == 1)
                    w = filter_sweep_f64<true>(reinterpret_cast<const double *>(slot_mem[1]), lane, op, c);
                else
                    w = filter_sweep_f64<false>(static_cast<const double *>(cols.data[f]) + tile * kFilterTile, lane, op, c);
            } else {
                const uint32_t *codes = slot == 0   ? reinterpret_cast<const uint32_t *>(slot_mem[0])
                                        : slot == 1 ? reinterpret_cast<const uint32_t *>(slot_mem[1])
                                                    : static_cast<const uint32_t *>(cols.data[f]) + tile * kFilterTile;
                if (op == VG_FILTER_EQ) {
                    const uint32_t c = static_cast<uint32_t>(uniform_i32(static_cast<int>(cl.code)));
                    w = filter_sweep(codes, lane, [c](uint32_t v) { return v == c; });
                } else if (op == VG_FILTER_IN) {
                    const int sb = uniform_i32(cl.set_begin), sc = uniform_i32(cl.set_count);
                    if (sb >= 0 && sc > 0 && sc <= kFilterMaxSet && static_cast<int64_t>(sb) + sc <= n_sets) {
                        int n2 = 1;
                        while (n2 < sc) n2 <<= 1;
                        for (int i = lane; i < n2; i += kWave) my_set[i] = i < sc ? sets[sb + i] : VG_INVALID_ID;
                        __threadfence_block();
                        filter_wave_sort(my_set, n2, lane);
                        const uint32_t *set = my_set;
                        w = filter_sweep(codes, lane, [set, n2](uint32_t v) { return filter_in_set(set, n2, v); });
                        __threadfence_block();  // the next clause's set is written behind these reads
                    }
                }
                // (a row without a value holds VG_INVALID_ID: the column's presence words, made at upload, clear it)
            }
            acc &= w & present;
        }
        const int64_t byte0 = word * 8;
        uint8_t *qm = mask + q * mask_stride;
        if (byte0 + 8 <= nbytes && word_stores) {
            *reinterpret_cast<uint64_t *>(qm + byte0) = acc;
        } else {
#pragma unroll
            for (int b = 0; b < 8; b++)
                if (byte0 + b < nbytes) qm[byte0 + b] = static_cast<uint8_t>(acc >> (8 * b));
        }
        if (counts) {
            const int c = wave_sum(__popcll(acc));
            if (lane == 0 && c) atomicAdd(counts + q, static_cast<unsigned long long>(c));
        }
    }
}

// bit r of word w <- row w * 64 + r has a code: the presence bitmap of a code column
__global__ __launch_bounds__(256) void filter_code_presence_kernel(const uint32_t *__restrict__ codes, int64_t padded_rows,
                                                                   uint64_t *__restrict__ present)
{
    const int lane = threadIdx.x & 63;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < padded_rows; i += static_cast<int64_t>(gridDim.x) * 256) {
        const uint64_t b = __ballot(codes[i] != VG_INVALID_ID);
        if (lane == 0) present[i >> 6] = b;
    }
}

__device__ __forceinline__ uint64_t mask_op(int op, uint64_t d, uint64_t s)
{
    return op == VG_MASK_AND ? d & s : op == VG_MASK_ANDNOT ? d & ~s : op == VG_MASK_OR ? d | s : d ^ s;
}

// dst[q] <- dst[q] op src[q] over nbytes bytes; 8-byte words where `words` says every address is aligned, bytes otherwise
__global__ __launch_bounds__(256) void mask_combine_kernel(int op, uint8_t *__restrict__ dst, int64_t dst_stride,
                                                           const uint8_t *__restrict__ src, int64_t src_stride, int64_t nbytes, int words)
{
    uint8_t *d = dst + static_cast<int64_t>(blockIdx.y) * dst_stride;
    const uint8_t *s = src + static_cast<int64_t>(blockIdx.y) * src_stride;
    const int64_t t0 = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x, step = static_cast<int64_t>(gridDim.x) * 256;
    const int64_t nwords = words ? nbytes >> 3 : 0;
    for (int64_t i = t0; i < nwords; i += step) {
        uint64_t *dw = reinterpret_cast<uint64_t *>(d) + i;
        *dw = mask_op(op, *dw, reinterpret_cast<const uint64_t *>(s)[i]);
    }
    for (int64_t i = nwords * 8 + t0; i < nbytes; i += step) d[i] = static_cast<uint8_t>(mask_op(op, d[i], s[i]));
}

// counts[q] <- the set bits below `rows` of query q's mask; one workgroup per query
__global__ __launch_bounds__(256) void mask_popcount_kernel(const uint8_t *__restrict__ mask, int64_t mask_stride, int64_t rows, int words,
                                                            long long *__restrict__ counts)
{
    __shared__ long long wsum[4];
    const uint8_t *m = mask + static_cast<int64_t>(blockIdx.x) * mask_stride;
    const int64_t full = rows >> 3;  // whole bytes; the last byte's bits at or above `rows` are not rows
    const int64_t nwords = words ? full >> 3 : 0;
    long long c = 0;
    for (int64_t i = threadIdx.x; i < nwords; i += 256) c += __popcll(reinterpret_cast<const uint64_t *>(m)[i]);
    for (int64_t i = nwords * 8 + threadIdx.x; i < full; i += 256) c += __popc(static_cast<uint32_t>(m[i]));
    if (threadIdx.x == 0 && (rows & 7)) c += __popc(static_cast<uint32_t>(m[full]) & ((1u << (rows & 7)) - 1u));
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

inline bool aligned8(const void *p, int64_t stride) { return ((reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(stride)) & 7) == 0; }

// A batch of masks that may live on the host: nq runs of nbytes bytes, `stride` apart.  A host batch is staged densely
// (runs 8-byte aligned); only the runs travel, so the caller's bytes between them are never touched.
struct MaskBatch {
    uint8_t *ptr = nullptr;
    int64_t stride = 0;
    uint8_t *host = nullptr;
    int64_t host_stride = 0, nq = 0, nbytes = 0;
    DevTmp<uint8_t> tmp;
    hipStream_t st = nullptr;
    int32_t init(const uint8_t *p, int64_t p_stride, int64_t nq_, int64_t nbytes_, bool copy_in, hipStream_t s)
    {
        st = s;
        nq = nq_;
        nbytes = nbytes_;
        ptr = const_cast<uint8_t *>(p);
        stride = p_stride;
        if (!p || nq == 0 || nbytes == 0 || is_device_ptr(p)) return VG_OK;
        host = ptr;
        host_stride = p_stride;
        const int64_t runs = p_stride == 0 ? 1 : nq;
        stride = p_stride == 0 ? 0 : (nbytes + 7) & ~int64_t(7);
        VG_TRY(tmp.init(static_cast<size_t>(runs) * ((nbytes + 7) & ~int64_t(7)), s));
        ptr = tmp.ptr;
        if (copy_in)
            VG_HIP(hipMemcpy2DAsync(ptr, (nbytes + 7) & ~int64_t(7), host, runs > 1 ? host_stride : nbytes, nbytes, runs,
                                    hipMemcpyHostToDevice, s));
        return VG_OK;
    }
    int32_t copy_out()
    {
        if (!host) return VG_OK;
        const int64_t runs = host_stride == 0 ? 1 : nq;
        VG_HIP(hipMemcpy2DAsync(host, runs > 1 ? host_stride : nbytes, ptr, (nbytes + 7) & ~int64_t(7), nbytes, runs,
                                hipMemcpyDeviceToHost, st));
        return VG_OK;
    }
};

const char *const kOpNames[] = {"eq", "ne", "lt", "lte", "gt", "gte", "in"};

// what the host can refuse about one clause it can read
int32_t filter_check_clause(const vg_columns *cols, const vg_filter_clause &cl, int64_t q, int64_t n_sets)
{
    VG_CHECK(cl.field >= 0 && cl.field < 64, VG_ERR_INVALID_ARG, "vg_filter_evaluate: query %lld names field %d, fields are 0..63",
             (long long)q, cl.field);
    VG_CHECK(cl.op >= VG_FILTER_EQ && cl.op <= VG_FILTER_IN, VG_ERR_INVALID_ARG, "vg_filter_evaluate: query %lld has unknown op %d",
             (long long)q, cl.op);
    const int kind = cols->col[cl.field].kind;
    VG_CHECK(!(kind == kColF64 && cl.op == VG_FILTER_IN), VG_ERR_UNSUPPORTED,
             "vg_filter_evaluate: query %lld: `in` on the f64 column of field %d", (long long)q, cl.field);
    VG_CHECK(!(kind == kColCodes && cl.op != VG_FILTER_EQ && cl.op != VG_FILTER_IN), VG_ERR_UNSUPPORTED,
             "vg_filter_evaluate: query %lld: `%s` on the code column of field %d (eq and in only)", (long long)q, kOpNames[cl.op], cl.field);
    if (cl.op == VG_FILTER_IN) {
        VG_CHECK(cl.set_count <= kFilterMaxSet, VG_ERR_UNSUPPORTED, "vg_filter_evaluate: query %lld: an `in` set of %d codes, at most %d",
                 (long long)q, cl.set_count, kFilterMaxSet);
        VG_CHECK(cl.set_begin >= 0 && cl.set_count >= 0 && static_cast<int64_t>(cl.set_begin) + cl.set_count <= n_sets, VG_ERR_INVALID_ARG,
                 "vg_filter_evaluate: query %lld: set range [%d, +%d) outside the %lld codes of `sets`", (long long)q, cl.set_begin,
                 cl.set_count, (long long)n_sets);
    }
    return VG_OK;
}

int32_t filter_run(vg_columns *cols, const vg_filter_clause *clauses, const int32_t *clause_off, int64_t nq, const uint32_t *sets,
                   int64_t n_sets, const uint8_t *deleted, uint8_t *mask, int64_t mask_stride, int64_t *counts, hipStream_t st)
{
    const int64_t rows = cols->rows, nbytes = (rows + 7) / 8;
    // the offsets and clauses the host can read are checked here; arrays in device memory are the caller's to keep well
    // formed (the kernel reads no clause beyond 16 per query and no set outside `sets`, and matches nothing there)
    const bool off_host = !is_device_ptr(clause_off), cl_host = clauses && !is_device_ptr(clauses);
    std::vector<int32_t> off_copy;
    const int32_t *off = clause_off;
    if (!off_host && cl_host) {  // the clause count is behind the offsets: read them back (a host buffer makes the call wait)
        off_copy.resize(static_cast<size_t>(nq) + 1);
        VG_HIP(hipMemcpyAsync(off_copy.data(), clause_off, off_copy.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        VG_HIP(hipStreamSynchronize(st));
        off = off_copy.data();
    }
    int64_t total = -1;
    if (off_host || cl_host) {
        VG_CHECK(off[0] >= 0, VG_ERR_INVALID_ARG, "vg_filter_evaluate: clause_off[0] = %d is negative", off[0]);
        for (int64_t q = 0; q < nq; q++) {
            VG_CHECK(off[q + 1] >= off[q], VG_ERR_INVALID_ARG, "vg_filter_evaluate: clause_off is not monotone at query %lld (%d after %d)",
                     (long long)q, off[q + 1], off[q]);
            VG_CHECK(off[q + 1] - off[q] <= kFilterMaxClauses, VG_ERR_UNSUPPORTED,
                     "vg_filter_evaluate: query %lld has %d clauses, at most %d", (long long)q, off[q + 1] - off[q], kFilterMaxClauses);
        }
        total = off[nq];
        VG_CHECK(total == 0 || clauses, VG_ERR_INVALID_ARG, "vg_filter_evaluate: %lld clauses but clauses is NULL", (long long)total);
    }
    if (cl_host) {
        for (int64_t q = 0; q < nq; q++)
            for (int32_t i = off[q]; i < off[q + 1]; i++) VG_TRY(filter_check_clause(cols, clauses[i], q, n_sets));
    }
    if (rows == 0) {  // no row: no mask byte; every count is 0
        if (counts) {
            DevOut<int64_t> cnt;
            VG_TRY(cnt.init(counts, static_cast<size_t>(nq), st, kAnyAlign));
            VG_HIP(hipMemsetAsync(cnt.ptr, 0, static_cast<size_t>(nq) * sizeof(int64_t), st));
            VG_TRY(cnt.finish());
        }
        return VG_OK;
    }

    DevIn<int32_t> d_off;
    VG_TRY(d_off.init(clause_off, static_cast<size_t>(nq) + 1, st, kAnyAlign));
    DevIn<vg_filter_clause> d_cl;
    if (cl_host) {
        if (total > 0) VG_TRY(d_cl.init(clauses, static_cast<size_t>(total), st, kAnyAlign));
    } else {
        d_cl.ptr = clauses;
    }
    DevIn<uint32_t> d_sets;
    VG_TRY(d_sets.init(sets, static_cast<size_t>(n_sets), st, kAnyAlign));
    // the deleted bitmap as whole words of whole tiles, wherever it lay
    DevTmp<uint64_t> d_del;
    if (deleted) {
        VG_TRY(d_del.init(static_cast<size_t>(cols->tiles) * 64, st));
        VG_HIP(hipMemsetAsync(d_del.ptr, 0, static_cast<size_t>(cols->tiles) * 64 * sizeof(uint64_t), st));
        VG_HIP(hipMemcpyAsync(d_del.ptr, deleted, static_cast<size_t>(nbytes), hipMemcpyDefault, st));
    }
    MaskBatch out;
    VG_TRY(out.init(mask, mask_stride, nq, nbytes, false, st));
    DevOut<int64_t> cnt;
    VG_TRY(cnt.init(counts, static_cast<size_t>(nq), st, kAnyAlign));
    if (counts) VG_HIP(hipMemsetAsync(cnt.ptr, 0, static_cast<size_t>(nq) * sizeof(int64_t), st));

    FilterCols fc;
    for (int f = 0; f < 64; f++) {
        fc.data[f] = cols->col[f].data;
        fc.present[f] = cols->col[f].present;
        fc.kind[f] = static_cast<uint8_t>(cols->col[f].kind);
    }
    // enough workgroups for every CU twice over, each with at least 32 queries (8 per wave) to spread a tile's staging over
    const int64_t want_y = std::max<int64_t>(1, (1024 + cols->tiles - 1) / cols->tiles);
    const int64_t staged_y = (nq + kFilterStageQueries - 1) / kFilterStageQueries;  // a chunk's offsets fit their LDS table
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(std::min<int64_t>(want_y, (nq + 31) / 32), staged_y), 65535));
    const int q_chunk = static_cast<int>((nq + chunks - 1) / chunks);
    const dim3 grid(static_cast<unsigned>(cols->tiles), static_cast<unsigned>((nq + q_chunk - 1) / q_chunk));
    {
        ProfScope p(cols->ctx, "filter_eval", st);
        VG_LAUNCH(filter_eval_kernel, grid, dim3(kFilterThreads), 0, st, fc, d_cl.ptr, d_off.ptr, nq, q_chunk, d_sets.ptr, n_sets, d_del.ptr,
                  rows, out.ptr, out.stride, aligned8(out.ptr, out.stride) ? 1 : 0, reinterpret_cast<unsigned long long *>(cnt.ptr));
    }
    VG_TRY(out.copy_out());
    VG_TRY(cnt.finish());
    const bool any_host = off_host || cl_host || out.host || cnt.host || (sets && n_sets > 0 && !is_device_ptr(sets)) ||
                          (deleted && !is_device_ptr(deleted));
    if (any_host) VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}

int32_t columns_set(vg_columns *cols, int32_t field, int kind, const void *values, const uint8_t *present, hipStream_t st)
{
    vg_columns::Col &c = cols->col[field];
    const size_t elem = kind == kColF64 ? sizeof(double) : sizeof(uint32_t);
    const size_t padded = static_cast<size_t>(cols->tiles) * kFilterTile;
    DevBuf<uint8_t> data;
    DevBuf<uint64_t> pres;
    VG_TRY(data.alloc(padded * elem));
    // rows past the end hold 0 / VG_INVALID_ID: never rows of a mask (the kernel's valid bits), never read out of bounds
    VG_HIP(hipMemsetAsync(data.p, kind == kColF64 ? 0 : 0xFF, std::max<size_t>(padded * elem, 1), st));
    if (cols->rows > 0) VG_HIP(hipMemcpyAsync(data.p, values, static_cast<size_t>(cols->rows) * elem, hipMemcpyDefault, st));
    if (kind == kColCodes) {
        VG_TRY(pres.alloc(padded / 64));
        if (padded > 0) {
            const unsigned grid = static_cast<unsigned>(std::min<size_t>(padded / 256, 2048));
            VG_LAUNCH(filter_code_presence_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(data.p),
                      static_cast<int64_t>(padded), pres.p);
        }
    } else if (present) {
        VG_TRY(pres.alloc(padded / 64));
        VG_HIP(hipMemsetAsync(pres.p, 0, std::max<size_t>(padded / 8, 8), st));
        if (cols->rows > 0) VG_HIP(hipMemcpyAsync(pres.p, present, static_cast<size_t>((cols->rows + 7) / 8), hipMemcpyDefault, st));
    }
    VG_HIP(hipStreamSynchronize(st));  // the caller's buffers are free again; work that read the old column is done
    drop_device(&c.data);
    drop_device(&c.present);
    c.data = data.release();
    c.present = pres.p ? pres.release() : nullptr;
    c.kind = kind;
    return VG_OK;
}

}  // namespace
}  // namespace vg

VG_API int32_t vg_columns_create(vg_ctx *ctx, int64_t rows, vg_columns **out)
{
    if (out) *out = nullptr;
    VG_CHECK(ctx && out, VG_ERR_INVALID_ARG, "vg_columns_create: NULL argument");
    VG_CHECK(rows >= 0, VG_ERR_INVALID_ARG, "vg_columns_create: rows = %lld is negative", (long long)rows);
    VG_CHECK(rows < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "vg_columns_create: %lld rows, fewer than 2^31 are supported", (long long)rows);
    vg_columns *cols = new vg_columns();
    cols->ctx = ctx;
    cols->rows = rows;
    cols->tiles = (rows + vg::kFilterTile - 1) / vg::kFilterTile;
    *out = cols;
    return VG_OK;
}

VG_API int32_t vg_columns_destroy(vg_columns *cols)
{
    if (!cols) return VG_OK;
    (void)hipSetDevice(cols->ctx->device);
    for (auto &c : cols->col) {
        vg::drop_device(&c.data);
        vg::drop_device(&c.present);
    }
    delete cols;
    return VG_OK;
}

VG_API int32_t vg_columns_set_f64(vg_columns *cols, int32_t field, const double *values, const uint8_t *present, void *stream)
{
    VG_CHECK(cols, VG_ERR_INVALID_ARG, "vg_columns_set_f64: NULL columns");
    VG_CHECK(field >= 0 && field < 64, VG_ERR_INVALID_ARG, "vg_columns_set_f64: field %d, fields are 0..63", field);
    VG_CHECK(values || cols->rows == 0, VG_ERR_INVALID_ARG, "vg_columns_set_f64: NULL values");
    VG_HIP(hipSetDevice(cols->ctx->device));
    return vg::columns_set(cols, field, vg::kColF64, values, present, vg::pick_stream(cols->ctx, stream));
}

VG_API int32_t vg_columns_set_codes(vg_columns *cols, int32_t field, const uint32_t *codes, void *stream)
{
    VG_CHECK(cols, VG_ERR_INVALID_ARG, "vg_columns_set_codes: NULL columns");
    VG_CHECK(field >= 0 && field < 64, VG_ERR_INVALID_ARG, "vg_columns_set_codes: field %d, fields are 0..63", field);
    VG_CHECK(codes || cols->rows == 0, VG_ERR_INVALID_ARG, "vg_columns_set_codes: NULL codes");
    VG_HIP(hipSetDevice(cols->ctx->device));
    return vg::columns_set(cols, field, vg::kColCodes, codes, nullptr, vg::pick_stream(cols->ctx, stream));
}

VG_API int32_t vg_columns_drop(vg_columns *cols, int32_t field)
{
    VG_CHECK(cols, VG_ERR_INVALID_ARG, "vg_columns_drop: NULL columns");
    VG_CHECK(field >= 0 && field < 64, VG_ERR_INVALID_ARG, "vg_columns_drop: field %d, fields are 0..63", field);
    VG_HIP(hipSetDevice(cols->ctx->device));
    vg_columns::Col &c = cols->col[field];
    if (c.kind != vg::kColNone) VG_HIP(hipDeviceSynchronize());  // an evaluation on any stream may still read it
    vg::drop_device(&c.data);
    vg::drop_device(&c.present);
    c.kind = vg::kColNone;
    return VG_OK;
}

VG_API int32_t vg_filter_evaluate(vg_columns *cols, const vg_filter_clause *clauses, const int32_t *clause_off, int64_t nq,
                                  const uint32_t *sets, int64_t n_sets, const uint8_t *deleted, uint8_t *mask, int64_t mask_stride,
                                  int64_t *counts, void *stream)
{
    VG_CHECK(cols, VG_ERR_INVALID_ARG, "vg_filter_evaluate: NULL columns");
    VG_CHECK(nq >= 0 && n_sets >= 0, VG_ERR_INVALID_ARG, "vg_filter_evaluate: nq = %lld, n_sets = %lld: negative", (long long)nq,
             (long long)n_sets);
    if (nq == 0) return VG_OK;
    VG_CHECK(nq < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "vg_filter_evaluate: %lld queries, fewer than 2^31 are supported", (long long)nq);
    VG_CHECK(clause_off, VG_ERR_INVALID_ARG, "vg_filter_evaluate: NULL clause_off");
    VG_CHECK(sets || n_sets == 0, VG_ERR_INVALID_ARG, "vg_filter_evaluate: n_sets = %lld but sets is NULL", (long long)n_sets);
    const int64_t nbytes = (cols->rows + 7) / 8;
    VG_CHECK(mask || cols->rows == 0, VG_ERR_INVALID_ARG, "vg_filter_evaluate: NULL mask");
    VG_CHECK(mask_stride >= nbytes || (mask_stride == 0 && nq <= 1), VG_ERR_INVALID_ARG,
             "vg_filter_evaluate: mask_stride = %lld, a query's mask has %lld bytes (0 only for a single query)", (long long)mask_stride,
             (long long)nbytes);
    VG_HIP(hipSetDevice(cols->ctx->device));
    return vg::filter_run(cols, clauses, clause_off, nq, sets, n_sets, deleted, mask, mask_stride, counts,
                          vg::pick_stream(cols->ctx, stream));
}

VG_API int32_t vg_mask_combine(vg_ctx *ctx, int32_t op, uint8_t *dst, int64_t dst_stride, const uint8_t *src, int64_t src_stride, int64_t nq,
                               int64_t rows, void *stream)
{
    VG_CHECK(ctx, VG_ERR_INVALID_ARG, "vg_mask_combine: NULL context");
    VG_CHECK(op >= VG_MASK_AND && op <= VG_MASK_XOR, VG_ERR_INVALID_ARG, "vg_mask_combine: unknown op %d", op);
    VG_CHECK(nq >= 0 && rows >= 0, VG_ERR_INVALID_ARG, "vg_mask_combine: nq = %lld, rows = %lld: negative", (long long)nq, (long long)rows);
    const int64_t nbytes = (rows + 7) / 8;
    if (nq == 0 || nbytes == 0) return VG_OK;
    VG_CHECK(nq <= 65535, VG_ERR_UNSUPPORTED, "vg_mask_combine: %lld queries, at most 65535 per call", (long long)nq);
    VG_CHECK(dst && src, VG_ERR_INVALID_ARG, "vg_mask_combine: NULL mask");
    VG_CHECK(dst_stride >= nbytes || (dst_stride == 0 && nq == 1), VG_ERR_INVALID_ARG,
             "vg_mask_combine: dst_stride = %lld, a query's mask has %lld bytes", (long long)dst_stride, (long long)nbytes);
    VG_CHECK(src_stride >= nbytes || src_stride == 0, VG_ERR_INVALID_ARG, "vg_mask_combine: src_stride = %lld, a query's mask has %lld bytes",
             (long long)src_stride, (long long)nbytes);
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = vg::pick_stream(ctx, stream);
    vg::MaskBatch d, s;
    VG_TRY(d.init(dst, dst_stride, nq, nbytes, true, st));
    VG_TRY(s.init(src, src_stride, nq, nbytes, true, st));
    const int words = vg::aligned8(d.ptr, d.stride) && vg::aligned8(s.ptr, s.stride) ? 1 : 0;
    const unsigned gx = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((nbytes / 8 + 255) / 256, 256)));
    {
        vg::ProfScope p(ctx, "mask_combine", st);
        VG_LAUNCH(vg::mask_combine_kernel, dim3(gx, static_cast<unsigned>(nq)), dim3(256), 0, st, op, d.ptr, d.stride, s.ptr, s.stride, nbytes,
                  words);
    }
    VG_TRY(d.copy_out());
    if (d.host || s.host) VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}

VG_API int32_t vg_mask_popcount(vg_ctx *ctx, const uint8_t *mask, int64_t mask_stride, int64_t nq, int64_t rows, int64_t *counts,
                                void *stream)
{
    VG_CHECK(ctx, VG_ERR_INVALID_ARG, "vg_mask_popcount: NULL context");
    VG_CHECK(nq >= 0 && rows >= 0, VG_ERR_INVALID_ARG, "vg_mask_popcount: nq = %lld, rows = %lld: negative", (long long)nq, (long long)rows);
    if (nq == 0) return VG_OK;
    VG_CHECK(nq < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "vg_mask_popcount: %lld queries, fewer than 2^31 are supported", (long long)nq);
    const int64_t nbytes = (rows + 7) / 8;
    VG_CHECK(counts && (mask || nbytes == 0), VG_ERR_INVALID_ARG, "vg_mask_popcount: NULL mask or counts");
    VG_CHECK(mask_stride >= nbytes || mask_stride == 0, VG_ERR_INVALID_ARG, "vg_mask_popcount: mask_stride = %lld, a query's mask has %lld bytes",
             (long long)mask_stride, (long long)nbytes);
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = vg::pick_stream(ctx, stream);
    vg::MaskBatch m;
    VG_TRY(m.init(mask, mask_stride, nq, nbytes, true, st));
    vg::DevOut<int64_t> cnt;
    VG_TRY(cnt.init(counts, static_cast<size_t>(nq), st, vg::kAnyAlign));
    {
        vg::ProfScope p(ctx, "mask_popcount", st);
        VG_LAUNCH(vg::mask_popcount_kernel, dim3(static_cast<unsigned>(nq)), dim3(256), 0, st, m.ptr, m.stride, rows, vg::aligned8(m.ptr, m.stride) ? 1 : 0,
                  reinterpret_cast<long long *>(cnt.ptr));
    }
    VG_TRY(cnt.finish());
    if (m.host) VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}

VG_API int32_t vg_mask_alloc(vg_ctx *ctx, int64_t bytes, uint8_t **out)
{
    if (out) *out = nullptr;
    VG_CHECK(ctx && out, VG_ERR_INVALID_ARG, "vg_mask_alloc: NULL argument");
    VG_CHECK(bytes >= 0, VG_ERR_INVALID_ARG, "vg_mask_alloc: bytes = %lld is negative", (long long)bytes);
    if (bytes == 0) return VG_OK;
    VG_HIP(hipSetDevice(ctx->device));
    vg::DevBuf<uint8_t> buf;
    VG_TRY(buf.alloc(static_cast<size_t>(bytes)));
    VG_HIP(hipMemset(buf.p, 0, static_cast<size_t>(bytes)));
    *out = buf.release();
    return VG_OK;
}

VG_API int32_t vg_mask_free(vg_ctx *ctx, uint8_t *mask)
{
    VG_CHECK(ctx, VG_ERR_INVALID_ARG, "vg_mask_free: NULL context");
    if (!mask) return VG_OK;
    VG_HIP(hipSetDevice(ctx->device));
    VG_HIP(hipFree(mask));
    return VG_OK;
}
