// k_flat_build.hip — flat.Writer.Flush (internal/segment/flat/writer.go:99-519) on a resident index.
//   vg_flat_build          the writer's partitioning (:105-169) and quantization (:171-223): TrainKMeans + AssignPartition are
//                          vg_kmeans_train / _assign on the resident rows, the counting sort (:132-153) is the stable grouping
//                          below, the rows / norms / bf16 image move through rb_permute_rows (vg_permute.hpp), the quantizer is
//                          trained and the codes are made from the reordered rows where they lie.  No row leaves the device.
//   vg_segment_write_flat  the file image (:312-470): header (format.go:28-56, :112-133), then the sections with no padding
//                          between them, the body's CRC-32C computed on the device for the sections that live there.
//   vg_crc32c_device       that CRC over any device byte range.
// Stable grouping (fg_*): a counting sort of the row ids by an 11-bit digit of the partition id — (1) a histogram per block of
//   consecutive rows (LDS counters; counts are order-free, so LDS atomics), (2) per digit a scan of its column over the blocks,
//   then a scan over the digits, (3) one wavefront per block places its rows 64 at a time: a row's rank among the rows of its
//   digit inside the 64 comes from ballots over the digit's bits, the block's running count per digit lives in LDS.  No global
//   atomic decides a position, so the order inside a partition is the rows' ascending original order: exactly a stable sort.
//   More than 2048 partitions: least-significant-digit passes (2 up to 4M partitions), each pass stable, keys re-read through
//   the previous pass's order.  The kernels read 4 B and write 4-8 B per row: at 1M rows they are launch-sized.
// CRC-32C (crc_*): a block covers 256 KiB as 16-byte pieces dealt round-robin to its 256 threads, so every load is coalesced;
//   a thread's register skips the 255 pieces between two of its own by one table operator (x^(8 * 4080), 4 lookups), takes its
//   piece by slicing-by-8 twice (16 lookups), is moved to the block's end by one product with a power of x and XORed with the
//   others.  Tables (13 KiB) in LDS.  The host chains the blocks' registers with vg::crc::combine (vg_crc32c.hpp).
#include <algorithm>
#include <mutex>
#include <vector>

#include "vg_crc32c.hpp"
#include "vg_crc_device.hpp"
#include "vg_internal.hpp"
#include "vg_permute.hpp"
#include "vg_segment_layout.hpp"

namespace vg {

// ---- the stable grouping ------------------------------------------------------------------------------------------------
constexpr int kFgDigitBits = 11;
constexpr int kFgBins = 1 << kFgDigitBits;  // LDS counters per block: 8 KiB
constexpr int64_t kFgMaxBlocks = 8192;

// the digit of row v's partition in this pass; nb = digits in use (a partition id outside [0, P) cannot index past a table)
__device__ __forceinline__ int fg_digit(const int32_t *__restrict__ assign, uint32_t v, int shift, int nb)
{
    const int d = static_cast<int>((static_cast<uint32_t>(assign[v]) >> shift) & (kFgBins - 1));
    return d < nb ? d : nb - 1;
}

// hist[block][d] = rows of the block whose digit is d; src: the rows' order so far (null: 0, 1, 2, ...)
__global__ __launch_bounds__(256) void fg_hist_kernel(const int32_t *__restrict__ assign, const uint32_t *__restrict__ src, int64_t n,
                                                      int64_t rpb, int shift, int nb, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[kFgBins];
    for (int d = threadIdx.x; d < nb; d += 256) h[d] = 0;
    __syncthreads();
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rpb, r1 = std::min(n, r0 + rpb);
    for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) atomicAdd(&h[fg_digit(assign, src ? src[i] : static_cast<uint32_t>(i), shift, nb)], 1u);
    __syncthreads();
    for (int d = threadIdx.x; d < nb; d += 256) hist[static_cast<int64_t>(blockIdx.x) * nb + d] = h[d];
}

// hist[block][d] becomes the digit-d rows of earlier blocks, counts[d] the digit's total: one workgroup per digit walks its
// column 256 blocks at a time
__global__ __launch_bounds__(kRbThreads) void fg_scan_blocks_kernel(uint32_t *__restrict__ hist, int blocks, int nb, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wsum[kRbThreads / 64];
    const int d = blockIdx.x;
    uint32_t carry = 0;
    for (int b0 = 0; b0 < blocks; b0 += kRbThreads) {
        const int b = b0 + threadIdx.x;
        const uint32_t v = b < blocks ? hist[static_cast<int64_t>(b) * nb + d] : 0u;
        uint32_t total;
        const uint32_t before = rb_block_scan(v, wsum, &total);
        if (b < blocks) hist[static_cast<int64_t>(b) * nb + d] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) counts[d] = carry;
}

// offsets[d] = rows of smaller digits (nb <= kFgBins = 8 per thread)
__global__ __launch_bounds__(kRbThreads) void fg_offsets_kernel(const uint32_t *__restrict__ counts, int nb, uint32_t *__restrict__ offsets)
{
    __shared__ uint32_t wsum[kRbThreads / 64];
    constexpr int per = kFgBins / kRbThreads;
    const int a = threadIdx.x * per;
    uint32_t sum = 0;
    for (int d = a; d < a + per && d < nb; d++) sum += counts[d];
    uint32_t total;
    uint32_t run = rb_block_scan(sum, wsum, &total);
    for (int d = a; d < a + per && d < nb; d++) {
        offsets[d] = run;
        run += counts[d];
    }
}

// one wavefront per block: dst[position] = row, and (the last pass) inv[row] = position
__global__ __launch_bounds__(64) void fg_place_kernel(const int32_t *__restrict__ assign, const uint32_t *__restrict__ src, int64_t n,
                                                      int64_t rpb, int shift, int nb, int bits, const uint32_t *__restrict__ hist,
                                                      const uint32_t *__restrict__ offsets, uint32_t *__restrict__ dst,
                                                      uint32_t *__restrict__ inv)
{
    __shared__ uint32_t base[kFgBins];
    const int lane = threadIdx.x;
    for (int d = lane; d < nb; d += 64) base[d] = offsets[d] + hist[static_cast<int64_t>(blockIdx.x) * nb + d];
    __syncthreads();
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rpb, r1 = std::min(n, r0 + rpb);
    for (int64_t c0 = r0; c0 < r1; c0 += 64) {
        const int64_t i = c0 + lane;
        const bool active = i < r1;
        const uint32_t v = active ? (src ? src[i] : static_cast<uint32_t>(i)) : 0u;
        const int d = active ? fg_digit(assign, v, shift, nb) : 0;
        unsigned long long peers = __ballot(active);
        for (int bit = 0; bit < bits; bit++) {
            const bool set = (d >> bit) & 1;
            const unsigned long long bb = __ballot(set);
            peers &= set ? bb : ~bb;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (active) {
            const uint32_t pos = base[d] + static_cast<uint32_t>(rank);
            if (pos < n) {  // (always, for partition ids in range)
                dst[pos] = v;
                if (inv) inv[v] = pos;
            }
        }
        __syncthreads();
        if (active && rank == 0) base[d] += static_cast<uint32_t>(__popcll(peers));
        __syncthreads();
    }
}

// part_off[p] = the first position whose row's partition is >= p, p = 0 .. P (part_off[P] = n)
__global__ __launch_bounds__(256) void fg_part_off_kernel(const int32_t *__restrict__ assign, const uint32_t *__restrict__ perm, int64_t n, int P,
                                                          uint32_t *__restrict__ part_off)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > P) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (assign[perm[mid]] < p)
            lo = mid + 1;
        else
            hi = mid;
    }
    part_off[p] = static_cast<uint32_t>(lo);
}

__global__ __launch_bounds__(256) void fg_iota_kernel(uint32_t *__restrict__ out, int64_t n)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256)
        out[i] = static_cast<uint32_t>(i);
}

// perm[new] = old, inv[old] = new, part_off[P + 1] from assign[n] in [0, P): the order of a stable sort by partition
static int32_t fg_group(const int32_t *assign, int64_t n, int P, uint32_t *perm, uint32_t *inv, uint32_t *part_off, hipStream_t st)
{
    int pbits = 0;
    while ((int64_t(1) << pbits) < P) pbits++;
    const int passes = std::max(1, (pbits + kFgDigitBits - 1) / kFgDigitBits);
    const int64_t rpb = std::max<int64_t>(2048, ((n + kFgMaxBlocks - 1) / kFgMaxBlocks + 63) / 64 * 64);
    const int blocks = static_cast<int>((n + rpb - 1) / rpb);
    DevTmp<uint32_t> hist, counts, offsets, tmp;
    VG_TRY(hist.init(static_cast<size_t>(blocks) * kFgBins, st));
    VG_TRY(counts.init(kFgBins, st));
    VG_TRY(offsets.init(kFgBins, st));
    if (passes > 1) VG_TRY(tmp.init(static_cast<size_t>(n), st));
    const uint32_t *src = nullptr;
    for (int j = 0; j < passes; j++) {
        const int shift = j * kFgDigitBits;
        const int nb = static_cast<int>(std::min<int64_t>(kFgBins, ((static_cast<int64_t>(P) - 1) >> shift) + 1));
        int bits = 0;
        while ((1 << bits) < nb) bits++;
        const bool last = j == passes - 1;
        uint32_t *dst = (passes - 1 - j) % 2 == 0 ? perm : tmp.ptr;
        VG_LAUNCH(fg_hist_kernel, dim3(blocks), dim3(256), 0, st, assign, src, n, rpb, shift, nb, hist.ptr);
        VG_LAUNCH(fg_scan_blocks_kernel, dim3(nb), dim3(kRbThreads), 0, st, hist.ptr, blocks, nb, counts.ptr);
        VG_LAUNCH(fg_offsets_kernel, dim3(1), dim3(kRbThreads), 0, st, counts.ptr, nb, offsets.ptr);
        VG_LAUNCH(fg_place_kernel, dim3(blocks), dim3(64), 0, st, assign, src, n, rpb, shift, nb, bits, hist.ptr, offsets.ptr, dst,
                  last ? inv : nullptr);
        src = dst;
    }
    VG_LAUNCH(fg_part_off_kernel, dim3((P + 1 + 255) / 256), dim3(256), 0, st, assign, perm, n, P, part_off);
    return VG_OK;
}

// ---- SQ8 codes back to the reference's row-major layout -----------------------------------------------------------------
// the inverse of sq8_retile_kernel (k_sq8_scan.hip): piece (tile, group, lane) -> codes[row * dim + group * 16 ...]
__global__ __launch_bounds__(256) void fg_sq8_untile_kernel(const uint4 *__restrict__ tiles, int64_t n, int dim, int groups, int64_t n_tiles,
                                                            uint8_t *__restrict__ codes)
{
    const int64_t total = n_tiles * groups * 64;
    for (int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; gid < total; gid += static_cast<int64_t>(gridDim.x) * 256) {
        const int lane = static_cast<int>(gid & 63);
        const int64_t tg = gid >> 6;
        const int g = static_cast<int>(tg % groups);
        const int64_t row = (tg / groups) * 64 + lane;
        if (row >= n) continue;
        const uint4 x = tiles[gid];
        uint8_t *dst = codes + row * dim + g * 16;
        if (dim % 16 == 0) {  // (codes is a 256-byte aligned scratch block)
            *reinterpret_cast<uint4 *>(dst) = x;
        } else {
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
            for (int b = 0; b < 16 && g * 16 + b < dim; b++) dst[b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
        }
    }
}

// ---- CRC-32C --------------------------------------------------------------------------------------------------------------
constexpr int kCrcThreads = 256;
constexpr int kCrcPerThread = 64;  // 16-byte pieces per thread: a block covers 256 KiB
constexpr int64_t kCrcBlockPieces = static_cast<int64_t>(kCrcThreads) * kCrcPerThread;
constexpr int64_t kCrcBlockBytes = kCrcBlockPieces * 16;

struct CrcTables {
    uint32_t slice[8][256];  // slicing-by-8 (vg_segment_layout.hpp's)
    uint32_t skip[4][256];   // register * x^(8 * 16 * (kCrcThreads - 1)), by register byte
    uint32_t tail[256];      // x^(8 * 16 * j)
};

__device__ __forceinline__ uint32_t crc_take8(const CrcTables &t, uint32_t c, uint32_t w0, uint32_t w1)
{
    const uint32_t lo = w0 ^ c, hi = w1;
    return t.slice[7][lo & 0xFF] ^ t.slice[6][(lo >> 8) & 0xFF] ^ t.slice[5][(lo >> 16) & 0xFF] ^ t.slice[4][lo >> 24] ^
           t.slice[3][hi & 0xFF] ^ t.slice[2][(hi >> 8) & 0xFF] ^ t.slice[1][(hi >> 16) & 0xFF] ^ t.slice[0][hi >> 24];
}

// out[block] = the raw register (init 0, no final xor) of the block's pieces; data: 16-byte aligned
__global__ __launch_bounds__(kCrcThreads) void crc_blocks_kernel(const uint4 *__restrict__ data, int64_t pieces, const CrcTables *__restrict__ tables,
                                                                 uint32_t *__restrict__ out)
{
    __shared__ CrcTables t;
    __shared__ uint32_t wsum[kCrcThreads / 64];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(tables);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&t);
        for (int i = threadIdx.x; i < static_cast<int>(sizeof(CrcTables) / 4); i += kCrcThreads) dst[i] = src[i];
    }
    __syncthreads();
    const int64_t p0 = static_cast<int64_t>(blockIdx.x) * kCrcBlockPieces;
    const int64_t mine = std::min<int64_t>(kCrcBlockPieces, pieces - p0);  // pieces of this block, >= 1
    const uint4 *base = data + p0;
    uint32_t c = 0;
    int64_t last = -1;
    for (int it0 = 0; it0 < kCrcPerThread; it0 += 4) {
        if (static_cast<int64_t>(it0) * kCrcThreads >= mine) break;  // (uniform)
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t p = static_cast<int64_t>(it0 + u) * kCrcThreads + threadIdx.x;
            v[u] = p < mine ? base[p] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t p = static_cast<int64_t>(it0 + u) * kCrcThreads + threadIdx.x;
            if (p >= mine) continue;
            if (last >= 0) c = t.skip[0][c & 0xFF] ^ t.skip[1][(c >> 8) & 0xFF] ^ t.skip[2][(c >> 16) & 0xFF] ^ t.skip[3][c >> 24];
            c = crc_take8(t, c, v[u].x, v[u].y);
            c = crc_take8(t, c, v[u].z, v[u].w);
            last = p;
        }
    }
    // to the block's end: the pieces after this thread's last one (fewer than kCrcThreads of them)
    if (last >= 0) c = crc::mulmod(t.tail[mine - 1 - last], c);
    for (int off = 32; off > 0; off >>= 1) c ^= __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = wsum[0] ^ wsum[1] ^ wsum[2] ^ wsum[3];
}

// the bytes in front of the first aligned piece and behind the last whole one (fewer than 16 each): out[0], out[1]
__global__ __launch_bounds__(64) void crc_edges_kernel(const uint8_t *__restrict__ head, int head_len, const uint8_t *__restrict__ tail, int tail_len,
                                                       const CrcTables *__restrict__ tables, uint32_t *__restrict__ out)
{
    if (threadIdx.x > 1) return;
    const uint8_t *p = threadIdx.x == 0 ? head : tail;
    const int len = threadIdx.x == 0 ? head_len : tail_len;
    uint32_t c = 0;
    for (int i = 0; i < len; i++) c = tables->slice[0][(c ^ p[i]) & 0xFF] ^ (c >> 8);
    out[threadIdx.x] = c;
}

int32_t crc_tables(int device, const CrcTables **out)
{
    static std::mutex mu;
    static const CrcTables *per_device[64] = {nullptr};
    VG_CHECK(device >= 0 && device < 64, VG_ERR_INVALID_ARG, "vg_crc32c_device: device %d", device);
    std::lock_guard<std::mutex> g(mu);
    if (!per_device[device]) {
        static const seglayout::Crc32cTables slicing;
        std::vector<CrcTables> h(1);
        memcpy(h[0].slice, slicing.t, sizeof h[0].slice);
        const uint32_t gap = crc::xpow8(16 * (kCrcThreads - 1));
        for (int j = 0; j < 4; j++)
            for (uint32_t b = 0; b < 256; b++) h[0].skip[j][b] = crc::mulmod(gap, b << (8 * j));
        for (int j = 0; j < 256; j++) h[0].tail[j] = crc::xpow8(16 * static_cast<uint64_t>(j));
        CrcTables *d = nullptr;  // 13 KiB per device, kept for the life of the process
        VG_HIP(hipMalloc(reinterpret_cast<void **>(&d), sizeof(CrcTables)));
        VG_HIP(hipMemcpy(d, h.data(), sizeof(CrcTables), hipMemcpyHostToDevice));
        per_device[device] = d;
    }
    *out = per_device[device];
    return VG_OK;
}

// CrcJob (vg_crc_device.hpp): one byte range's CRC in two steps
void CrcJob::plan(const void *ptr, int64_t bytes)
{
    size = bytes;
    head = std::min<int64_t>(bytes, static_cast<int64_t>((16 - (reinterpret_cast<uintptr_t>(ptr) & 15)) & 15));
    pieces = (bytes - head) / 16;
    tail = bytes - head - pieces * 16;
    blocks = (pieces + kCrcBlockPieces - 1) / kCrcBlockPieces;
}

int32_t CrcJob::launch(const void *ptr, const CrcTables *tables, uint32_t *d_out, hipStream_t st) const
{
    const uint8_t *p = static_cast<const uint8_t *>(ptr);
    VG_LAUNCH(crc_edges_kernel, dim3(1), dim3(64), 0, st, p, static_cast<int>(head), p + head + pieces * 16, static_cast<int>(tail), tables,
              d_out);
    if (blocks)
        VG_LAUNCH(crc_blocks_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kCrcThreads), 0, st, reinterpret_cast<const uint4 *>(p + head),
                  pieces, tables, d_out + 2);
    return VG_OK;
}

uint32_t CrcJob::finish(const uint32_t *h_out) const
{
    const uint32_t full = crc::xpow8(static_cast<uint64_t>(kCrcBlockBytes));
    uint32_t acc = h_out[0];
    for (int64_t b = 0; b < blocks; b++) {
        const int64_t bytes = std::min(kCrcBlockPieces, pieces - b * kCrcBlockPieces) * 16;
        acc = crc::mulmod(bytes == kCrcBlockBytes ? full : crc::xpow8(static_cast<uint64_t>(bytes)), acc) ^ h_out[2 + b];
    }
    return crc::combine(acc, h_out[1], static_cast<uint64_t>(tail));
}

// ---- the image's layout (writer.go:312-345) -----------------------------------------------------------------------------
struct FlatImage {
    int qtype = 0;  // format.go:22-26
    uint64_t rows = 0, centroids = 0, part_off = 0, quant = 0, codes = 0, vectors = 0, ids = 0, metadata = 0, stats = 0;  // section bytes
    uint64_t total() const { return seglayout::kFlatHeader + centroids + part_off + quant + codes + vectors + ids + metadata + stats; }
};

static int uvarint_len(uint64_t v)
{
    int l = 1;
    for (; v >= 0x80; v >>= 7) l++;
    return l;
}

// the sections' sizes; metadata_bytes / stats_bytes < 0: what the writer emits when no row has a document
static int32_t flat_image_plan(const vg_index *idx, int64_t metadata_bytes, int64_t stats_bytes, FlatImage &L, const char *fn)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(!idx->d_hnsw_l0 && !idx->d_vamana, VG_ERR_UNSUPPORTED, "%s: the index holds a graph: not a flat segment", fn);
    VG_CHECK(!idx->d_rq_rows && !idx->d_rq_tiles && !idx->d_int4_rows, VG_ERR_UNSUPPORTED,
             "%s: the flat format has no quantization type for %s codes (format.go:22-26)", fn, idx->d_int4_rows ? "INT4" : "RaBitQ");
    const bool sq = idx->sq && idx->d_sq_tiles, pq = idx->pq && idx->d_pq_rows;
    VG_CHECK(!(sq && pq), VG_ERR_UNSUPPORTED, "%s: the index holds SQ8 and PQ codes, a flat segment has one kind", fn);
    VG_CHECK(!pq || idx->pq->k == 256, VG_ERR_UNSUPPORTED, "%s: the flat writer's PQ has 256 centroids (writer.go:204), this one %d", fn,
             idx->pq->k);
    VG_CHECK(idx->n == 0 || idx->d_vectors, VG_ERR_NOT_READY, "%s: index has no fp32 rows", fn);
    const uint64_t n = static_cast<uint64_t>(idx->n), dim = static_cast<uint64_t>(idx->dim), P = static_cast<uint64_t>(idx->num_partitions);
    L.rows = n;
    L.qtype = sq ? 1 : pq ? 2 : 0;
    L.centroids = P * dim * 4;
    L.part_off = P ? (P + 1) * 4 : 0;
    L.quant = sq ? dim * 8 : pq ? 8 + static_cast<uint64_t>(idx->pq->m) * 8 + static_cast<uint64_t>(idx->pq->m) * 256 * idx->pq->subdim : 0;
    L.codes = sq ? n * dim : pq ? n * idx->pq->m : 0;
    L.vectors = n * dim * 4;
    L.ids = n * 8;
    L.metadata = metadata_bytes >= 0 ? static_cast<uint64_t>(metadata_bytes) : n ? (n + 1) * 4 : 0;
    const uint64_t stat_blocks = (n + 1023) / 1024;  // format.go:14 BlockSize
    L.stats = stats_bytes >= 0 ? static_cast<uint64_t>(stats_bytes) : uvarint_len(stat_blocks) + 2 * stat_blocks;
    return VG_OK;
}

}  // namespace vg

VG_API int32_t vg_crc32c_device(vg_ctx *ctx, const void *device_ptr, int64_t size, uint32_t *out, void *stream)
{
    VG_CHECK(ctx && out, VG_ERR_INVALID_ARG, "vg_crc32c_device: NULL context or result");
    VG_CHECK(size >= 0 && (size == 0 || device_ptr), VG_ERR_INVALID_ARG, "vg_crc32c_device: NULL data or negative size");
    *out = 0;
    if (size == 0) return VG_OK;
    VG_CHECK(vg::is_device_ptr(device_ptr), VG_ERR_INVALID_ARG, "vg_crc32c_device: data is not device memory (vg_crc32c is the host's)");
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = vg::pick_stream(ctx, stream);
    const vg::CrcTables *tables;
    VG_TRY(vg::crc_tables(ctx->device, &tables));
    vg::CrcJob job;
    job.plan(device_ptr, size);
    vg::DevTmp<uint32_t> d;
    VG_TRY(d.init(job.words(), st));
    {
        vg::ProfScope prof(ctx, "crc32c_device", st);
        VG_TRY(job.launch(device_ptr, tables, d.ptr, st));
    }
    std::vector<uint32_t> h(job.words());
    VG_HIP(hipMemcpyAsync(h.data(), d.ptr, h.size() * 4, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    *out = vg::crc::finish_raw(job.finish(h.data()), static_cast<uint64_t>(size));
    return VG_OK;
}

VG_API int32_t vg_flat_build(vg_index *idx, int32_t num_partitions, int32_t quantization, int32_t pq_m, int32_t kmeans_iters, int32_t pq_iters,
                             uint64_t seed, vg_sq8 *sq, vg_pq *pq, uint32_t *perm, uint32_t *inv_perm, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_flat_build: NULL index");
    VG_CHECK(idx->n == 0 || idx->d_vectors, VG_ERR_NOT_READY, "vg_flat_build: index has no fp32 rows");
    VG_CHECK(idx->metric != VG_METRIC_HAMMING, VG_ERR_UNSUPPORTED, "unsupported metric for float32: %d", idx->metric);
    VG_CHECK(!idx->d_hnsw_l0 && !idx->d_hnsw_tomb && !idx->d_hnsw_l0_dist && !idx->d_vamana, VG_ERR_UNSUPPORTED,
             "vg_flat_build: the index holds %s, which the flat writer never has", idx->d_vamana ? "a Vamana graph" : "an HNSW graph");
    VG_CHECK(!idx->d_pq_tiles && !idx->d_pq_rows && !idx->d_sq_tiles && !idx->d_rq_rows && !idx->d_rq_tiles && !idx->d_int4_rows,
             VG_ERR_UNSUPPORTED, "vg_flat_build: the index holds codes already: the writer quantizes the reordered rows itself");
    VG_CHECK(!idx->d_centroids && idx->num_partitions == 0, VG_ERR_UNSUPPORTED, "vg_flat_build: the index is partitioned already");
    VG_CHECK(!idx->pq_nom.rows && !idx->sq_nom.rows, VG_ERR_UNSUPPORTED, "vg_flat_build: the index holds a nomination image");
    VG_CHECK(quantization == VG_QUANT_NONE || quantization == VG_QUANT_SQ8 || quantization == VG_QUANT_PQ, VG_ERR_INVALID_ARG,
             "vg_flat_build: quantization %d is none of VG_QUANT_NONE / _SQ8 / _PQ (format.go:22-26)", quantization);
    VG_CHECK(kmeans_iters >= 0 && pq_iters >= 0 && pq_m >= 0, VG_ERR_INVALID_ARG, "vg_flat_build: negative iteration count or pq_m");
    VG_CHECK(quantization != VG_QUANT_SQ8 || sq, VG_ERR_INVALID_ARG, "vg_flat_build: VG_QUANT_SQ8 without a vg_sq8");
    VG_CHECK(quantization != VG_QUANT_PQ || pq, VG_ERR_INVALID_ARG, "vg_flat_build: VG_QUANT_PQ without a vg_pq");
    if (quantization == VG_QUANT_SQ8) VG_CHECK(sq->dim == idx->dim, VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
    if (quantization == VG_QUANT_PQ) {
        VG_CHECK(pq->dim == idx->dim, VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        const int32_t want_m = pq_m ? pq_m : idx->dim / 8;  // writer.go:66
        VG_CHECK(pq->m == want_m && pq->k == 256, VG_ERR_INVALID_ARG,
                 "vg_flat_build: the vg_pq has m = %d, k = %d; the writer's is NewProductQuantizer(dim, %d, 256) (writer.go:204)", pq->m, pq->k,
                 want_m);
        VG_TRY(vg::pq_train_refusal(pq, idx->n));  // before anything moves
    }
    const int64_t n = idx->n;
    if (n == 0) return VG_OK;
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int32_t dim = idx->dim;
    const bool partition = num_partitions > 1 && n >= num_partitions;  // writer.go:105
    vg::DevTmp<uint32_t> order, inv;
    VG_TRY(order.init(static_cast<size_t>(n), st));
    if (partition) {
        const int P = num_partitions;
        vg::DevTmp<float> cent;
        vg::DevTmp<int32_t> assign;
        vg::DevTmp<uint32_t> part_off;
        VG_TRY(cent.init(static_cast<size_t>(P) * dim, st));
        VG_TRY(assign.init(static_cast<size_t>(n), st));
        VG_TRY(inv.init(static_cast<size_t>(n), st));
        VG_TRY(part_off.init(static_cast<size_t>(P) + 1, st));
        int32_t produced = 0;
        VG_TRY(vg_kmeans_train(idx->ctx, idx->d_vectors, n, dim, P, idx->metric, kmeans_iters ? kmeans_iters : 10, seed, cent.ptr, &produced,
                               stream));  // writer.go:109
        VG_CHECK(produced, VG_ERR_HIP, "vg_flat_build: k-means produced no centroids");
        VG_TRY(vg_kmeans_assign(idx->ctx, idx->d_vectors, n, dim, cent.ptr, P, idx->metric, assign.ptr, stream));  // :117-125
        {
            vg::ProfScope prof(idx->ctx, "flat_build_group", st);
            VG_TRY(vg::fg_group(assign.ptr, n, P, order.ptr, inv.ptr, part_off.ptr, st));  // :132-165
        }
        {
            vg::ProfScope prof(idx->ctx, "flat_build_permute", st);
            const int64_t bf16_bytes = static_cast<int64_t>(idx->vectors_bf16_dim) * 2;
            const int64_t scratch_bytes = n * std::max<int64_t>(static_cast<int64_t>(dim) * 4, idx->d_vectors_bf16 ? bf16_bytes : 0);
            void *scratch = nullptr;
            VG_HIP(hipMalloc(&scratch, static_cast<size_t>(scratch_bytes)));
            struct Free {
                void *p;
                hipStream_t st;
                ~Free()
                {
                    (void)hipStreamSynchronize(st);
                    (void)hipFree(p);
                }
            } free_scratch{scratch, st};
            VG_TRY(vg::rb_permute_rows(idx->d_vectors, n, static_cast<int64_t>(dim) * 4, order.ptr, scratch, st));
            VG_TRY(vg::rb_permute_rows(idx->d_norms, n, 4, order.ptr, scratch, st));
            VG_TRY(vg::rb_permute_rows(idx->d_vectors_bf16, n, bf16_bytes, order.ptr, scratch, st));
        }
        VG_TRY(vg_index_set_partitions(idx, cent.ptr, part_off.ptr, P, stream));
    } else {
        VG_LAUNCH(vg::fg_iota_kernel, dim3(vg::rb_grid(n)), dim3(256), 0, st, order.ptr, n);
    }
    if (perm) VG_HIP(hipMemcpyAsync(perm, order.ptr, static_cast<size_t>(n) * 4, hipMemcpyDefault, st));
    if (inv_perm) VG_HIP(hipMemcpyAsync(inv_perm, partition ? inv.ptr : order.ptr, static_cast<size_t>(n) * 4, hipMemcpyDefault, st));
    VG_HIP(hipStreamSynchronize(st));
    // quantization over the reordered rows (writer.go:171-223)
    if (quantization == VG_QUANT_SQ8) {
        vg::DevTmp<uint8_t> codes;
        VG_TRY(codes.init(static_cast<size_t>(n) * dim, st));
        VG_TRY(vg_sq8_train(sq, idx->d_vectors, n, stream));
        VG_TRY(vg_sq8_encode(sq, idx->d_vectors, n, codes.ptr, stream));
        VG_TRY(vg_index_set_sq8_codes(idx, sq, codes.ptr, stream));
    } else if (quantization == VG_QUANT_PQ) {
        vg::DevTmp<uint8_t> codes;
        VG_TRY(codes.init(static_cast<size_t>(n) * pq->m, st));
        VG_TRY(vg_pq_train(pq, idx->d_vectors, n, pq_iters ? pq_iters : 20, seed, stream));
        VG_TRY(vg_pq_encode(pq, idx->d_vectors, n, codes.ptr, stream));
        VG_TRY(vg_index_set_pq_codes(idx, pq, codes.ptr, stream));
    }
    return VG_OK;
}

VG_API int64_t vg_segment_flat_image_size(const vg_index *idx, int64_t metadata_bytes, int64_t block_stats_bytes)
{
    vg::FlatImage L;
    if (vg::flat_image_plan(idx, metadata_bytes, block_stats_bytes, L, "vg_segment_flat_image_size") != VG_OK) return -1;
    return static_cast<int64_t>(L.total());
}

VG_API int32_t vg_segment_write_flat(vg_index *idx, uint64_t segment_id, const uint64_t *ids, const void *metadata_section,
                                     int64_t metadata_bytes, const void *block_stats, int64_t block_stats_bytes, void *image,
                                     int64_t image_size, int64_t *written, void *stream)
{
    using namespace vg::seglayout;
    if (written) *written = 0;
    vg::FlatImage L;
    VG_TRY(vg::flat_image_plan(idx, metadata_section ? metadata_bytes : -1, block_stats ? block_stats_bytes : -1, L, "vg_segment_write_flat"));
    VG_CHECK(image, VG_ERR_INVALID_ARG, "vg_segment_write_flat: image is NULL");
    VG_CHECK((!metadata_section || metadata_bytes >= 0) && (!block_stats || block_stats_bytes >= 0), VG_ERR_INVALID_ARG,
             "vg_segment_write_flat: negative section size");
    VG_CHECK(image_size >= 0 && static_cast<uint64_t>(image_size) >= L.total(), VG_ERR_INVALID_ARG,
             "vg_segment_write_flat: the image needs %llu bytes, the buffer has %lld", static_cast<unsigned long long>(L.total()),
             static_cast<long long>(image_size));
    VG_CHECK(idx->n <= 0xFFFFFFFFll, VG_ERR_UNSUPPORTED, "vg_segment_write_flat: RowCount is a uint32");
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int64_t n = idx->n;
    const int32_t dim = idx->dim;
    uint8_t *img = static_cast<uint8_t *>(image);
    // writer.go:335-345: every offset is the running position, present or not
    const uint64_t o_cent = kFlatHeader, o_poff = o_cent + L.centroids, o_quant = o_poff + L.part_off, o_codes = o_quant + L.quant,
                   o_vec = o_codes + L.codes, o_ids = o_vec + L.vectors, o_meta = o_ids + L.ids, o_stats = o_meta + L.metadata;

    // the device's share of the checksum: codes and rows, virtually every byte of the body
    const vg::CrcTables *tables = nullptr;
    vg::CrcJob job_codes, job_rows;
    vg::DevTmp<uint32_t> d_crc;
    vg::DevTmp<uint8_t> sq_rows;
    const uint8_t *d_codes = nullptr;
    if (n) {
        VG_TRY(vg::crc_tables(idx->ctx->device, &tables));
        if (L.qtype == 1) {  // the index keeps SQ8 codes tiled: back to rows
            VG_TRY(sq_rows.init(static_cast<size_t>(L.codes), st));
            VG_LAUNCH(vg::fg_sq8_untile_kernel, dim3(vg::rb_grid(idx->n_tiles * idx->sq_groups * 64)), dim3(256), 0, st,
                      reinterpret_cast<const uint4 *>(idx->d_sq_tiles), n, dim, idx->sq_groups, idx->n_tiles, sq_rows.ptr);
            d_codes = sq_rows.ptr;
        } else if (L.qtype == 2) {
            d_codes = idx->d_pq_rows;
        }
        job_codes.plan(d_codes, static_cast<int64_t>(L.codes));
        job_rows.plan(idx->d_vectors, static_cast<int64_t>(L.vectors));
        VG_TRY(d_crc.init(job_codes.words() + job_rows.words(), st));
        vg::ProfScope prof(idx->ctx, "crc32c_device", st);
        if (L.codes) VG_TRY(job_codes.launch(d_codes, tables, d_crc.ptr, st));
        VG_TRY(job_rows.launch(idx->d_vectors, tables, d_crc.ptr + job_codes.words(), st));
    }
    // the small device sections, then the host's own, and their CRCs, while those kernels run
    if (L.centroids) VG_HIP(hipMemcpyAsync(img + o_cent, idx->d_centroids, L.centroids, hipMemcpyDeviceToHost, st));
    if (L.qtype == 1) {
        VG_HIP(hipMemcpyAsync(img + o_quant, idx->sq->d_mins, L.quant, hipMemcpyDeviceToHost, st));  // mins then maxs: one block
    } else if (L.qtype == 2) {
        const uint64_t m = static_cast<uint64_t>(idx->pq->m);
        wr32(img + o_quant, static_cast<uint32_t>(m));
        wr32(img + o_quant + 4, 256u);
        VG_HIP(hipMemcpyAsync(img + o_quant + 8, idx->pq->d_scales, m * 4, hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(img + o_quant + 8 + m * 4, idx->pq->d_offsets, m * 4, hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(img + o_quant + 8 + m * 8, idx->pq->d_codebooks, m * 256 * idx->pq->subdim, hipMemcpyDeviceToHost, st));
    }
    if (L.part_off) memcpy(img + o_poff, idx->h_part_off.data(), L.part_off);
    for (int64_t i = 0; i < n; i++) wr64(img + o_ids + 8 * static_cast<uint64_t>(i), ids ? ids[i] : static_cast<uint64_t>(i));
    if (metadata_section) {
        if (L.metadata) memcpy(img + o_meta, metadata_section, L.metadata);
    } else {
        memset(img + o_meta, 0, L.metadata);  // rows + 1 zero offsets, no blob (writer.go:230-292 with every md nil)
    }
    if (block_stats) {
        if (L.stats) memcpy(img + o_stats, block_stats, L.stats);
    } else {  // uvarint(blocks), then per block uvarint(1) and the one byte of an empty field map (:294-307, format.go:58-71)
        uint8_t *p = img + o_stats;
        for (uint64_t v = (static_cast<uint64_t>(n) + 1023) / 1024;;) {
            if (v >= 0x80) {
                *p++ = static_cast<uint8_t>(v) | 0x80;
                v >>= 7;
            } else {
                *p++ = static_cast<uint8_t>(v);
                break;
            }
        }
        for (; p < img + o_stats + L.stats; p += 2) {
            p[0] = 1;
            p[1] = 0;
        }
    }
    std::vector<uint32_t> h_crc(n ? job_codes.words() + job_rows.words() : 0);
    if (n) VG_HIP(hipMemcpyAsync(h_crc.data(), d_crc.ptr, h_crc.size() * 4, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));  // the small sections are in the image
    uint32_t crc = 0;  // of the body so far
    crc = vg::crc::combine(crc, vg_crc32c(img + o_cent, static_cast<int64_t>(o_codes - o_cent)), o_codes - o_cent);
    // the big sections go home while the host checksums its own
    if (L.codes) VG_HIP(hipMemcpyAsync(img + o_codes, d_codes, L.codes, hipMemcpyDeviceToHost, st));
    if (L.vectors) VG_HIP(hipMemcpyAsync(img + o_vec, idx->d_vectors, L.vectors, hipMemcpyDeviceToHost, st));
    if (n) {
        if (L.codes) crc = vg::crc::combine(crc, vg::crc::finish_raw(job_codes.finish(h_crc.data()), L.codes), L.codes);
        crc = vg::crc::combine(crc, vg::crc::finish_raw(job_rows.finish(h_crc.data() + job_codes.words()), L.vectors), L.vectors);
    }
    const uint64_t rest = L.ids + L.metadata + L.stats;
    crc = vg::crc::combine(crc, vg_crc32c(img + o_ids, static_cast<int64_t>(rest)), rest);
    // the header (format.go:112-133)
    memset(img, 0, kFlatHeader);
    wr32(img, kFlatMagic);
    wr32(img + 4, 1);
    wr64(img + 8, segment_id);
    wr32(img + 16, static_cast<uint32_t>(n));
    wr32(img + 20, static_cast<uint32_t>(dim));
    img[24] = static_cast<uint8_t>(idx->metric);
    wr32(img + 28, static_cast<uint32_t>(idx->num_partitions));
    img[32] = static_cast<uint8_t>(L.qtype);
    wr64(img + 40, o_cent);
    wr64(img + 48, o_poff);
    wr64(img + 56, o_quant);
    wr64(img + 64, o_codes);
    wr64(img + 72, o_vec);
    wr64(img + 80, o_ids);
    wr64(img + 88, o_meta);
    wr64(img + 96, o_stats);
    wr32(img + 104, crc);
    VG_HIP(hipStreamSynchronize(st));
    if (written) *written = static_cast<int64_t>(L.total());
    return VG_OK;
}
