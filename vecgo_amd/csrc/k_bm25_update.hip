// k_bm25_update.hip — writes to a resident BM25 index (vg_bm25.hpp) without a rebuild:
//
//   vg_bm25_update        a batch of MemoryIndex.deleteLocked (bm25.go:238-278) followed by a batch of Add (:180-229), applied
//                         to the CSR image where it lies
//   vg_bm25_create_empty  the index such updates fill;  vg_bm25_export  the image copied out
//
// The next image is built beside the current one (the postings and the offsets each ping-pong between two buffers), so a
// failed call leaves the index as it was.  All work is per posting, never per term: a list of a million postings and a list
// of one cost the same per element.  kChunk = VG_BM25_UPDATE_CHUNK old postings belong to one workgroup in both passes over
// them.
//
//   live     a bitmap of the deleted docs; every chunk: a live bit per old posting, the chunk's live count and the count in
//            front of every 32 postings of it.  One workgroup turns the chunk counts into offsets (prefix_kernel).  The
//            live rank of ANY old posting is then three loads (live_rank): a term's live length is the difference of the
//            ranks at its two ends of term_off.
//   order    the added postings arrive document-major; they become 64-bit (term << 32 | doc) keys with tf as the payload and
//            go through an LSD radix sort, 8 bits a pass, stable inside a pass; the digits that are zero for every term below
//            n_terms_new and every doc below n_docs_new are skipped.  (There is no single-workgroup LDS form: a small batch
//            costs a few short launches beside a pass over every posting of the index.)
//   offsets  new length of a list = live + added; a two-level scan over n_terms_new gives the new term_off and the offsets
//            of the terms' runs in the sorted added postings.
//   merge    by position, no comparison loop: a live old posting goes to new_off[t] + its live rank inside its list + the
//            added postings of t with a smaller doc (a search in t's short run); an added posting goes to new_off[t] + its
//            rank in the run + the live rank of the lower bound of its doc in t's old list.  An equal, live doc at that lower
//            bound is an add into a live slot: the error flag.  A workgroup finds the terms of its chunk's first and last
//            posting once; a thread then looks for the next term only where its postings cross a boundary, inside that range.
//   docs     after the flag and the new offsets have been read back (the call's one wait): doc_len / doc_to_id of the deleted
//            docs, then of the added ones.
#include <algorithm>
#include <vector>

#include "vg_bm25.hpp"
#include "vg_device.hpp"
#include "vg_internal.hpp"
#include "vg_scan.hpp"

namespace vg {
namespace {

constexpr int kChunk = VG_BM25_UPDATE_CHUNK;  // old postings of one workgroup: kScanThreads threads, kPer consecutive postings each
constexpr int kPer = 8;
static_assert(kChunk == kScanThreads * kPer, "a thread owns eight consecutive postings of the chunk");
constexpr int kGroups = kChunk / 32;          // 32-posting groups of a chunk: one word of live bits and one count each
constexpr int kSortChunk = 2048;              // added postings of one (single-wave) workgroup of a radix pass
constexpr int kSortRounds = kSortChunk / 64;
constexpr int kTermsPerBlock = kScanThreads;  // terms of one workgroup of the offset scan

enum UpdateError : unsigned long long { kErrNone = 0, kErrLiveSlot = 1, kErrDoc = 2, kErrTerm = 3 };

// err[0] <- code, err[1] <- value, for the first caller only
__device__ __forceinline__ void raise(unsigned long long *err, unsigned long long code, unsigned long long value)
{
    if (atomicCAS(&err[0], 0ull, code) == 0ull) err[1] = value;
}

// What the live pass leaves: chunk_off[c] = live postings in front of chunk c (chunks + 1 entries), sub[g] = live postings of
// g's chunk in front of 32-posting group g, bits[g] = the group's live bits (chunks * kGroups + 1 entries each, the last 0)
struct LiveRank {
    const int64_t *chunk_off;
    const uint32_t *sub, *bits;
    // live old postings in front of posting q, 0 <= q <= n_post
    __device__ __forceinline__ int64_t operator()(int64_t q) const
    {
        const int64_t g = q >> 5;
        return chunk_off[q / kChunk] + sub[g] + __popc(bits[g] & ((1u << (q & 31)) - 1u));
    }
    __device__ __forceinline__ bool live(int64_t q) const { return (bits[q >> 5] >> (q & 31)) & 1u; }
};

// the first i of lo .. hi with a[i] >= key (a ascending)
template <typename T, typename K>
__device__ __forceinline__ int64_t lower_bound_dev(const T *__restrict__ a, int64_t lo, int64_t hi, K key)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (static_cast<K>(a[mid]) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the last t of lo .. hi - 1 with off[t] <= p (off ascending, off[lo] <= p)
__device__ __forceinline__ int64_t owner_of(const int64_t *__restrict__ off, int64_t lo, int64_t hi, int64_t p)
{
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- docs of the call: the deleted docs' bitmap, the ids of both lists checked ---------------------------------------------
__global__ __launch_bounds__(256) void bm25u_mark_docs_kernel(const uint32_t *__restrict__ del_docs, int64_t n_del, int64_t n_docs_old,
                                                              uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ add_docs, int64_t n_add,
                                                              int64_t n_docs_new, unsigned long long *__restrict__ err)
{
    const int64_t step = static_cast<int64_t>(gridDim.x) * blockDim.x, i0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < n_del; i += step) {
        const uint32_t d = del_docs[i];
        if (d >= n_docs_old) raise(err, kErrDoc, d);
        else atomicOr(&bitmap[d >> 5], 1u << (d & 31));
    }
    for (int64_t i = i0; i < n_add; i += step)
        if (add_docs[i] >= n_docs_new) raise(err, kErrDoc, add_docs[i]);
}

// the eight docs of this thread; full: the chunk lies inside the list, two 16-byte loads
__device__ __forceinline__ void load8(const uint32_t *__restrict__ a, int64_t p0, int64_t n, bool full, uint32_t (&v)[kPer])
{
    if (full) {
        const uint4 x = *reinterpret_cast<const uint4 *>(a + p0), y = *reinterpret_cast<const uint4 *>(a + p0 + 4);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w, v[4] = y.x, v[5] = y.y, v[6] = y.z, v[7] = y.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPer; j++) v[j] = p0 + j < n ? a[p0 + j] : 0u;
    }
}

// ---- live: one workgroup per chunk of old postings -----------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void bm25u_live_kernel(const uint32_t *__restrict__ post_doc, int64_t n_post, const uint32_t *__restrict__ bitmap,
                                                                  uint32_t n_docs, uint32_t *__restrict__ bits, uint32_t *__restrict__ sub, int64_t *__restrict__ chunk_cnt)
{
    __shared__ long long wsum[kScanThreads / 64];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x, c0 = c * kChunk, p0 = c0 + static_cast<int64_t>(tid) * kPer;
    uint32_t m = 0;
    if (bitmap) {
        uint32_t d[kPer];
        load8(post_doc, p0, n_post, c0 + kChunk <= n_post, d);
#pragma unroll
        for (int j = 0; j < kPer; j++)
            if (p0 + j < n_post && !(d[j] < n_docs && ((bitmap[d[j] >> 5] >> (d[j] & 31)) & 1u))) m |= 1u << j;
    } else {  // nothing is deleted: every posting lives
        const int64_t left = n_post - p0;
        m = left >= kPer ? 0xFFu : left > 0 ? (1u << left) - 1u : 0u;
    }
    const int cnt = __popc(m);
    long long total;
    const long long inc = block_scan(cnt, wsum, total);
    uint32_t w = m;  // the group's word: the masks of its four threads
    w |= __shfl_down(w, 1) << 8;
    w |= __shfl_down(w, 2) << 16;
    if ((tid & 3) == 0) {
        const int64_t g = c * kGroups + (tid >> 2);
        bits[g] = w;
        sub[g] = static_cast<uint32_t>(inc - cnt);
    }
    if (tid == 0) chunk_cnt[c] = total;
}

// ---- order: keys of the added postings, then LSD radix passes ---------------------------------------------------------------
__global__ __launch_bounds__(256) void bm25u_keys_kernel(const int64_t *__restrict__ add_off, int64_t n_add, const uint32_t *__restrict__ add_docs,
                                                         const uint32_t *__restrict__ add_terms, const uint32_t *__restrict__ add_tf, int64_t n_addp,
                                                         int64_t n_docs_new, int64_t n_terms_new, uint64_t *__restrict__ keys, uint32_t *__restrict__ tfs,
                                                         uint32_t *__restrict__ add_cnt, unsigned long long *__restrict__ err)
{
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < n_addp; p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t i = owner_of(add_off, 0, n_add, p);  // the doc whose postings hold p
        uint32_t term = add_terms[p], doc = add_docs[i];
        if (term >= n_terms_new) {  // (device arrays are not validated: the call fails, and nothing is written out of range)
            raise(err, kErrTerm, term);
            term = static_cast<uint32_t>(n_terms_new - 1);
        }
        if (doc >= n_docs_new) doc = static_cast<uint32_t>(n_docs_new - 1);  // (flagged by bm25u_mark_docs_kernel)
        keys[p] = (static_cast<uint64_t>(term) << 32) | doc;
        tfs[p] = add_tf[p];
        atomicAdd(&add_cnt[term], 1u);
    }
}

// hist[digit * chunks + chunk] <- the keys of the chunk with that digit; one wave per chunk
__global__ __launch_bounds__(64) void bm25u_radix_hist_kernel(const uint64_t *__restrict__ keys, int64_t n, int shift, uint32_t *__restrict__ hist,
                                                              int64_t chunks)
{
    __shared__ uint32_t h[256];
    const int lane = threadIdx.x;
    for (int d = lane; d < 256; d += 64) h[d] = 0;
    __syncthreads();
    const int64_t c0 = static_cast<int64_t>(blockIdx.x) * kSortChunk;
    for (int r = 0; r < kSortRounds; r++) {
        const int64_t p = c0 + r * 64 + lane;
        if (p < n) atomicAdd(&h[(keys[p] >> shift) & 0xFF], 1u);
    }
    __syncthreads();
    for (int d = lane; d < 256; d += 64) hist[d * chunks + blockIdx.x] = h[d];
}

// hist holds each digit's exclusive prefix over the chunks, digit_total the digits' totals: the chunk's keys go behind
// (keys with a smaller digit) + (keys of the digit in earlier chunks) + (keys of the digit earlier in this chunk): stable
__global__ __launch_bounds__(64) void bm25u_radix_scatter_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ tfs, int64_t n, int shift,
                                                                 const uint32_t *__restrict__ hist, const int64_t *__restrict__ digit_total, int64_t chunks,
                                                                 uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_tfs)
{
    __shared__ uint32_t base[256];
    const int lane = threadIdx.x;
    {
        uint32_t t[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            t[j] = sum;
            sum += static_cast<uint32_t>(digit_total[lane * 4 + j]);
        }
        uint32_t inc = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) base[lane * 4 + j] = inc - sum + t[j] + hist[(lane * 4 + j) * chunks + blockIdx.x];
    }
    __syncthreads();
    const int64_t c0 = static_cast<int64_t>(blockIdx.x) * kSortChunk;
    for (int r = 0; r < kSortRounds; r++) {
        const int64_t p = c0 + r * 64 + lane;
        const bool valid = p < n;
        const uint64_t key = valid ? keys[p] : 0;
        const uint32_t tf = valid ? tfs[p] : 0;
        const uint32_t digit = static_cast<uint32_t>(key >> shift) & 0xFF;
        uint64_t peers = __ballot(valid);  // the lanes of this round with my digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint64_t has = __ballot((digit >> b) & 1u);
            peers &= ((digit >> b) & 1u) ? has : ~has;
        }
        const uint32_t at = valid ? base[digit] + __popcll(peers & ((uint64_t(1) << lane) - 1)) : 0u;
        __syncthreads();  // every lane has read base
        if (valid) {
            if (at < n) {
                out_keys[at] = key;
                out_tfs[at] = tf;
            }
            if ((peers & ((uint64_t(1) << lane) - 1)) == 0) base[digit] += __popcll(peers);  // the digit's first lane of the round
        }
        __syncthreads();
    }
}

// ---- offsets: a two-level scan over the new terms ---------------------------------------------------------------------------
// new_off[t] / add_off_t[t] <- the exclusive prefix INSIDE the block of (live + added) / added; block_sum[b], block_sum[blocks + b]
__global__ __launch_bounds__(kScanThreads) void bm25u_term_len_kernel(const int64_t *__restrict__ term_off, int64_t n_terms_old, int64_t n_terms_new,
                                                                      LiveRank lr, const uint32_t *__restrict__ add_cnt, int64_t *__restrict__ new_off,
                                                                      int64_t *__restrict__ run_off, int64_t *__restrict__ block_sum, int64_t blocks)
{
    __shared__ long long wsum[kScanThreads / 64];
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kTermsPerBlock + threadIdx.x;
    const long long live = t < n_terms_old ? lr(term_off[t + 1]) - lr(term_off[t]) : 0;
    const long long added = t < n_terms_new ? add_cnt[t] : 0;
    long long total_len, total_add;
    const long long inc_len = block_scan(live + added, wsum, total_len);
    const long long inc_add = block_scan(added, wsum, total_add);
    if (t < n_terms_new) {
        new_off[t] = inc_len - (live + added);
        run_off[t] = inc_add - added;
    }
    if (threadIdx.x == 0) {
        block_sum[blockIdx.x] = total_len;
        block_sum[blocks + blockIdx.x] = total_add;
    }
}

// block_sum holds its two halves' exclusive prefixes, total[2] their totals
__global__ __launch_bounds__(kScanThreads) void bm25u_term_fix_kernel(int64_t *__restrict__ new_off, int64_t *__restrict__ run_off, int64_t n_terms_new,
                                                                      const int64_t *__restrict__ block_sum, int64_t blocks, const int64_t *__restrict__ total)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kTermsPerBlock + threadIdx.x;
    if (t < n_terms_new) {
        new_off[t] += block_sum[blockIdx.x];
        run_off[t] += block_sum[blocks + blockIdx.x];
    } else if (t == n_terms_new) {
        new_off[t] = total[0];
        run_off[t] = total[1];
    }
}

struct MergeArgs {
    const int64_t *term_off;  // the old image
    const uint32_t *post_doc, *post_tf;
    int64_t n_post, n_terms_old;
    LiveRank lr;
    const int64_t *new_off, *run_off;  // n_terms_new + 1 each
    const uint64_t *keys;              // the added postings in (term, doc) order
    const uint32_t *tfs;
    int64_t n_addp;
    uint32_t *out_doc, *out_tf;
    int64_t out_cap;
};

// ---- merge, old side: one workgroup per chunk ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void bm25u_merge_old_kernel(MergeArgs a)
{
    __shared__ long long wsum[kScanThreads / 64];
    __shared__ int64_t range_s[2];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x, c0 = c * kChunk, c1 = min(c0 + kChunk, a.n_post), p0 = c0 + static_cast<int64_t>(tid) * kPer;
    if (tid < 2) range_s[tid] = owner_of(a.term_off, 0, a.n_terms_old, tid == 0 ? c0 : c1 - 1);  // the terms of the chunk's first and last posting
    const bool full = c0 + kChunk <= a.n_post;
    uint32_t d[kPer], tf[kPer];
    load8(a.post_doc, p0, a.n_post, full, d);
    load8(a.post_tf, p0, a.n_post, full, tf);
    const uint32_t m = p0 < a.n_post ? (a.lr.bits[p0 >> 5] >> ((tid & 3) * 8)) & 0xFFu : 0u;
    const int cnt = __popc(m);
    long long total;
    const long long inc = block_scan(cnt, wsum, total);  // (its barriers publish range_s)
    if (m == 0) return;
    int64_t rank = a.lr.chunk_off[c] + inc - cnt;        // the live rank of this thread's next live posting
    const int64_t t_last = range_s[1];
    int64_t t = range_s[0], t_end = -1, dst0 = 0, run0 = 0, run1 = 0;  // the current term: its end in the old list, new_off - its first live rank, its run
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        if (!((m >> j) & 1u)) continue;
        const int64_t p = p0 + j;
        if (p >= t_end) {  // a boundary was crossed (or the first live posting): the next term, looked for inside the chunk's range
            t = owner_of(a.term_off, t, t_last + 1, p);
            t_end = a.term_off[t + 1];
            dst0 = a.new_off[t] - a.lr(a.term_off[t]);
            run0 = a.run_off[t];
            run1 = a.run_off[t + 1];
        }
        int64_t smaller = 0;  // the term's added postings in front of this doc
        if (run1 > run0) smaller = lower_bound_dev(a.keys, run0, run1, (static_cast<uint64_t>(t) << 32) | d[j]) - run0;
        const int64_t dst = dst0 + rank + smaller;
        if (dst < a.out_cap) {
            a.out_doc[dst] = d[j];
            a.out_tf[dst] = tf[j];
        }
        rank++;
    }
}

// ---- merge, added side: one thread per added posting ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bm25u_merge_add_kernel(MergeArgs a, unsigned long long *__restrict__ err)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n_addp; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const uint64_t key = a.keys[i];
        const int64_t t = static_cast<int64_t>(key >> 32);
        const uint32_t doc = static_cast<uint32_t>(key);
        int64_t live_before = 0;  // live postings of t's old list with a smaller doc
        if (t < a.n_terms_old) {
            const int64_t lo = a.term_off[t], hi = a.term_off[t + 1];
            const int64_t q = lower_bound_dev(a.post_doc, lo, hi, doc);
            if (q < hi && a.post_doc[q] == doc && a.lr.live(q)) raise(err, kErrLiveSlot, doc);  // an add into a live slot
            live_before = a.lr(q) - a.lr(lo);
        }
        const int64_t dst = a.new_off[t] + (i - a.run_off[t]) + live_before;
        if (dst < a.out_cap) {
            a.out_doc[dst] = doc;
            a.out_tf[dst] = a.tfs[i];
        }
    }
}

// ---- docs: deleted, then added ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bm25u_docs_del_kernel(const uint32_t *__restrict__ del_docs, int64_t n_del, uint32_t *__restrict__ doc_len,
                                                             uint32_t *__restrict__ doc_to_id)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_del; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        doc_len[del_docs[i]] = 0;                    // bm25.go:268
        if (doc_to_id) doc_to_id[del_docs[i]] = 0;   // :269
    }
}
__global__ __launch_bounds__(256) void bm25u_docs_add_kernel(const uint32_t *__restrict__ add_docs, const uint32_t *__restrict__ add_len,
                                                             const uint32_t *__restrict__ add_ids, int64_t n_add, uint32_t *__restrict__ doc_len,
                                                             uint32_t *__restrict__ doc_to_id)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_add; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        doc_len[add_docs[i]] = add_len[i];
        if (doc_to_id) doc_to_id[add_docs[i]] = add_ids[i];
    }
}

unsigned grid_for(int64_t n, int threads) { return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n + threads - 1) / threads, 16384))); }

// room for `need` elements in the spare half of a ping-pong pair (it holds nothing the index needs): grown by half at least
template <typename T>
int32_t spare_room(T **p, int64_t *cap, int64_t need, int64_t in_use)
{
    if (*p && *cap >= need) return VG_OK;
    const int64_t have = std::max(*cap, in_use);
    const int64_t want = std::max<int64_t>(std::max(need, have + have / 2), 1);
    DevBuf<T> q;
    VG_TRY(q.alloc(static_cast<size_t>(want)));
    drop_device(p);
    *p = q.release();
    *cap = want;
    return VG_OK;
}

// a per-doc array with room for n_new docs: its n_old values kept, the slots behind them 0
int32_t grow_docs(uint32_t **p, int64_t n_old, int64_t want, hipStream_t st)
{
    DevBuf<uint32_t> q;
    VG_TRY(q.alloc(static_cast<size_t>(want)));
    if (*p && n_old) VG_HIP(hipMemcpyAsync(q.p, *p, static_cast<size_t>(n_old) * 4, hipMemcpyDeviceToDevice, st));
    if (want > n_old) VG_HIP(hipMemsetAsync(q.p + n_old, 0, static_cast<size_t>(want - n_old) * 4, st));
    VG_HIP(hipStreamSynchronize(st));
    drop_device(p);
    *p = q.release();
    return VG_OK;
}

// what a caller's arrays in HOST memory must satisfy (vecgo_hip.h), each refusal naming the doc or the term
int32_t validate_host(const vg_bm25 *bm, const uint32_t *del_docs, int64_t n_del, const uint32_t *add_docs, int64_t n_add, const int64_t *h_add_off,
                      const uint32_t *add_terms, int64_t n_docs_new, int64_t n_terms_new)
{
    if (n_del && !is_device_ptr(del_docs))
        for (int64_t i = 0; i < n_del; i++)
            VG_CHECK(static_cast<int64_t>(del_docs[i]) < bm->n_docs, VG_ERR_INVALID_ARG, "vg_bm25_update: del_docs names doc %u, the index holds %lld",
                     del_docs[i], (long long)bm->n_docs);
    if (n_add && !is_device_ptr(add_docs)) {
        std::vector<uint32_t> sorted(add_docs, add_docs + n_add);
        std::sort(sorted.begin(), sorted.end());
        VG_CHECK(static_cast<int64_t>(sorted.back()) < n_docs_new, VG_ERR_INVALID_ARG, "vg_bm25_update: add_docs names doc %u, n_docs_new = %lld",
                 sorted.back(), (long long)n_docs_new);
        for (int64_t i = 1; i < n_add; i++)
            VG_CHECK(sorted[i] != sorted[i - 1], VG_ERR_INVALID_ARG, "vg_bm25_update: add_docs names doc %u twice", sorted[i]);
    }
    const int64_t n_addp = h_add_off[n_add];
    if (n_addp && !is_device_ptr(add_terms)) {
        const bool docs_on_host = !is_device_ptr(add_docs);
        std::vector<uint32_t> terms;
        for (int64_t i = 0; i < n_add; i++) {
            terms.assign(add_terms + h_add_off[i], add_terms + h_add_off[i + 1]);
            std::sort(terms.begin(), terms.end());
            for (size_t j = 0; j < terms.size(); j++) {
                VG_CHECK(static_cast<int64_t>(terms[j]) < n_terms_new, VG_ERR_INVALID_ARG, "vg_bm25_update: added doc %lld names term %u, n_terms_new = %lld",
                         (long long)(docs_on_host ? add_docs[i] : i), terms[j], (long long)n_terms_new);
                VG_CHECK(j == 0 || terms[j] != terms[j - 1], VG_ERR_INVALID_ARG, "vg_bm25_update: added doc %lld names term %u twice",
                         (long long)(docs_on_host ? add_docs[i] : i), terms[j]);
            }
        }
    }
    return VG_OK;
}

}  // namespace
}  // namespace vg

VG_API int32_t vg_bm25_create_empty(vg_ctx *ctx, int32_t with_doc_to_id, vg_bm25 **out)
{
    VG_CHECK(ctx && out, VG_ERR_INVALID_ARG, "vg_bm25_create_empty: NULL context or result");
    *out = nullptr;
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    vg_bm25 *bm = new vg_bm25();
    bm->ctx = ctx;
    bm->mapped = with_doc_to_id != 0;
    vg::bm25_set_constants(bm, 0, 0);
    bm->h_term_off.assign(1, 0);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&bm->d_term_off), sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&bm->d_replayed), sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(bm->d_term_off, 0, sizeof(int64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(bm->d_replayed, 0, sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        vg::set_error("vg_bm25_create_empty: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        (void)vg_bm25_destroy(bm);
        return e == hipErrorOutOfMemory ? VG_ERR_OUT_OF_MEMORY : VG_ERR_HIP;
    }
    *out = bm;
    return VG_OK;
}

VG_API int32_t vg_bm25_update(vg_bm25 *bm, const uint32_t *del_docs, int64_t n_del, const uint32_t *add_docs, const uint32_t *add_len,
                              const uint32_t *add_ids, int64_t n_add, const int64_t *add_off, const uint32_t *add_terms, const uint32_t *add_tf,
                              int64_t n_docs_new, int64_t n_terms_new, int64_t total_length, int64_t doc_count, void *stream)
{
    VG_CHECK(bm, VG_ERR_INVALID_ARG, "vg_bm25_update: NULL index");
    VG_CHECK(n_del >= 0 && n_add >= 0, VG_ERR_INVALID_ARG, "vg_bm25_update: n_del = %lld, n_add = %lld: negative", (long long)n_del, (long long)n_add);
    VG_CHECK(n_docs_new >= bm->n_docs, VG_ERR_INVALID_ARG, "vg_bm25_update: n_docs_new = %lld shrinks an index of %lld docs", (long long)n_docs_new,
             (long long)bm->n_docs);
    VG_CHECK(n_terms_new >= bm->n_terms, VG_ERR_INVALID_ARG, "vg_bm25_update: n_terms_new = %lld shrinks an index of %lld terms", (long long)n_terms_new,
             (long long)bm->n_terms);
    VG_CHECK(n_docs_new < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "vg_bm25_update: n_docs_new = %lld, fewer than 2^31 docs are supported",
             (long long)n_docs_new);
    VG_CHECK(n_terms_new < (int64_t(1) << 32) - 1, VG_ERR_UNSUPPORTED, "vg_bm25_update: n_terms_new = %lld, term ids are uint32", (long long)n_terms_new);
    VG_CHECK(total_length >= 0 && doc_count >= 0, VG_ERR_INVALID_ARG, "vg_bm25_update: total_length = %lld, doc_count = %lld: negative",
             (long long)total_length, (long long)doc_count);
    VG_CHECK(del_docs || n_del == 0, VG_ERR_INVALID_ARG, "vg_bm25_update: NULL del_docs");
    VG_CHECK((add_docs && add_len && add_off) || n_add == 0, VG_ERR_INVALID_ARG, "vg_bm25_update: NULL add_docs, add_len or add_off");
    VG_CHECK(!(add_ids && !bm->mapped), VG_ERR_INVALID_ARG, "vg_bm25_update: add_ids for an index that reports doc ids themselves (no doc_to_id)");
    VG_CHECK(add_ids || !bm->mapped || n_add == 0, VG_ERR_INVALID_ARG, "vg_bm25_update: the index reports through doc_to_id: add_ids is required");
    vg_ctx *ctx = bm->ctx;
    VG_HIP(hipSetDevice(ctx->device));
    hipStream_t st = vg::pick_stream(ctx, stream);

    // the added docs' posting ranges on the host: they size everything (device memory: read back, as vg_bm25_create reads term_off)
    std::vector<int64_t> off_store;
    const int64_t zero_off = 0, *h_add_off = &zero_off;
    if (n_add) VG_TRY(vg::host_view(add_off, static_cast<size_t>(n_add) + 1, st, off_store, h_add_off));
    VG_CHECK(h_add_off[0] == 0, VG_ERR_INVALID_ARG, "vg_bm25_update: add_off[0] = %lld, not 0", (long long)h_add_off[0]);
    for (int64_t i = 0; i < n_add; i++)
        VG_CHECK(h_add_off[i + 1] >= h_add_off[i], VG_ERR_INVALID_ARG, "vg_bm25_update: add_off decreases at added doc %lld", (long long)i);
    const int64_t n_addp = h_add_off[n_add];
    VG_CHECK(n_addp < (int64_t(1) << 31), VG_ERR_UNSUPPORTED, "vg_bm25_update: %lld added postings, fewer than 2^31 per call are supported",
             (long long)n_addp);
    VG_CHECK((add_terms && add_tf) || n_addp == 0, VG_ERR_INVALID_ARG, "vg_bm25_update: NULL add_terms or add_tf");
    VG_CHECK(n_addp == 0 || n_terms_new > 0, VG_ERR_INVALID_ARG, "vg_bm25_update: %lld added postings and n_terms_new = 0", (long long)n_addp);
    VG_CHECK(n_add == 0 || n_docs_new > 0, VG_ERR_INVALID_ARG, "vg_bm25_update: %lld added docs and n_docs_new = 0", (long long)n_add);
    VG_TRY(vg::validate_host(bm, del_docs, n_del, add_docs, n_add, h_add_off, add_terms, n_docs_new, n_terms_new));

    vg::DevIn<uint32_t> d_del, d_docs, d_len, d_ids, d_terms, d_tf;
    vg::DevIn<int64_t> d_off;
    VG_TRY(d_del.init(del_docs, static_cast<size_t>(n_del), st, vg::kAnyAlign));
    VG_TRY(d_docs.init(add_docs, static_cast<size_t>(n_add), st, vg::kAnyAlign));
    VG_TRY(d_len.init(add_len, static_cast<size_t>(n_add), st, vg::kAnyAlign));
    VG_TRY(d_ids.init(add_ids, static_cast<size_t>(n_add), st, vg::kAnyAlign));
    VG_TRY(d_off.init(add_off, n_add ? static_cast<size_t>(n_add) + 1 : 0, st, vg::kAnyAlign));
    VG_TRY(d_terms.init(add_terms, static_cast<size_t>(n_addp), st, vg::kAnyAlign));
    VG_TRY(d_tf.init(add_tf, static_cast<size_t>(n_addp), st, vg::kAnyAlign));

    // the next image's buffers: the spare halves, with room for every old and every added posting
    const int64_t n_post = bm->n_post, n_terms_old = bm->n_terms, n_docs_old = bm->n_docs;
    {
        int64_t cap_doc = bm->alt_post_cap, cap_tf = bm->alt_post_cap;  // (the two posting arrays grow together)
        VG_TRY(vg::spare_room(&bm->d_alt_doc, &cap_doc, n_post + n_addp, std::max(bm->post_cap, n_post)));
        VG_TRY(vg::spare_room(&bm->d_alt_tf, &cap_tf, n_post + n_addp, std::max(bm->post_cap, n_post)));
        bm->alt_post_cap = std::min(cap_doc, cap_tf);
    }
    VG_TRY(vg::spare_room(&bm->d_alt_off, &bm->alt_off_cap, n_terms_new + 1, std::max(bm->off_cap, n_terms_old + 1)));

    const int64_t chunks = (n_post + vg::kChunk - 1) / vg::kChunk, groups = chunks * vg::kGroups + 1;
    const int64_t sort_chunks = (n_addp + vg::kSortChunk - 1) / vg::kSortChunk;
    const int64_t term_blocks = (n_terms_new + vg::kTermsPerBlock - 1) / vg::kTermsPerBlock;
    vg::ArenaCall ar(ctx, st);
    const int i_state = ar.add(4 * 8);  // err[2], total[2]
    const int i_bitmap = ar.add(static_cast<size_t>((n_docs_old + 31) / 32 + 1) * 4);
    const int i_chunk = ar.add(static_cast<size_t>(chunks + 1) * 8);
    const int i_bits = ar.add(static_cast<size_t>(groups) * 4), i_sub = ar.add(static_cast<size_t>(groups) * 4);
    const int i_key0 = ar.add(static_cast<size_t>(n_addp + 1) * 8), i_key1 = ar.add(static_cast<size_t>(n_addp + 1) * 8);
    const int i_tf0 = ar.add(static_cast<size_t>(n_addp + 1) * 4), i_tf1 = ar.add(static_cast<size_t>(n_addp + 1) * 4);
    const int i_hist = ar.add(static_cast<size_t>(sort_chunks * 256 + 1) * 4), i_dtot = ar.add(256 * 8);
    const int i_cnt = ar.add(static_cast<size_t>(n_terms_new + 1) * 4), i_run = ar.add(static_cast<size_t>(n_terms_new + 1) * 8);
    const int i_bsum = ar.add(static_cast<size_t>(2 * term_blocks + 1) * 8);
    VG_TRY(ar.commit());
    unsigned long long *err = ar.get<unsigned long long>(i_state);
    int64_t *total = reinterpret_cast<int64_t *>(err + 2);
    uint32_t *bitmap = n_del ? ar.get<uint32_t>(i_bitmap) : nullptr;
    int64_t *chunk_off = ar.get<int64_t>(i_chunk);
    uint32_t *bits = ar.get<uint32_t>(i_bits), *sub = ar.get<uint32_t>(i_sub);
    uint64_t *key[2] = {ar.get<uint64_t>(i_key0), ar.get<uint64_t>(i_key1)};
    uint32_t *tf[2] = {ar.get<uint32_t>(i_tf0), ar.get<uint32_t>(i_tf1)};
    uint32_t *hist = ar.get<uint32_t>(i_hist), *add_cnt = ar.get<uint32_t>(i_cnt);
    int64_t *digit_total = ar.get<int64_t>(i_dtot), *run_off = ar.get<int64_t>(i_run), *block_sum = ar.get<int64_t>(i_bsum);
    const vg::LiveRank lr{chunk_off, sub, bits};

    VG_HIP(hipMemsetAsync(err, 0, 4 * 8, st));
    VG_HIP(hipMemsetAsync(chunk_off + chunks, 0, 8, st));
    VG_HIP(hipMemsetAsync(bits + groups - 1, 0, 4, st));
    VG_HIP(hipMemsetAsync(sub + groups - 1, 0, 4, st));
    VG_HIP(hipMemsetAsync(add_cnt, 0, static_cast<size_t>(n_terms_new + 1) * 4, st));
    {
        vg::ProfScope prof(ctx, "bm25_update_live", st);
        if (bitmap) VG_HIP(hipMemsetAsync(bitmap, 0, static_cast<size_t>((n_docs_old + 31) / 32 + 1) * 4, st));
        if (n_del || n_add)
            VG_LAUNCH(vg::bm25u_mark_docs_kernel, dim3(vg::grid_for(std::max(n_del, n_add), 256)), dim3(256), 0, st, d_del.ptr, n_del, n_docs_old, bitmap,
                      d_docs.ptr, n_add, n_docs_new, err);
        if (chunks)
            VG_LAUNCH(vg::bm25u_live_kernel, dim3(static_cast<unsigned>(chunks)), dim3(vg::kScanThreads), 0, st, bm->d_post_doc, n_post, bitmap,
                      static_cast<uint32_t>(n_docs_old), bits, sub,
                      chunk_off);
        VG_LAUNCH(vg::prefix_kernel<int64_t>, dim3(1), dim3(vg::kScanThreads), 0, st, chunk_off, chunks + 1, nullptr, nullptr);
    }
    int cur = 0;  // which of the two key buffers holds the added postings
    if (n_addp) {
        vg::ProfScope prof(ctx, "bm25_update_order", st);
        VG_LAUNCH(vg::bm25u_keys_kernel, dim3(vg::grid_for(n_addp, 256)), dim3(256), 0, st, d_off.ptr, n_add, d_docs.ptr, d_terms.ptr, d_tf.ptr, n_addp,
                  n_docs_new, n_terms_new, key[0], tf[0], add_cnt, err);
        // the digits of (term << 32 | doc) that can differ: those not 0 in the call's largest doc and term
        const uint64_t max_key = (static_cast<uint64_t>(n_terms_new - 1) << 32) | static_cast<uint64_t>(n_docs_new - 1);
        for (int digit = 0; digit < 8; digit++) {
            const int shift = digit * 8;
            const uint64_t half = digit < 4 ? (max_key & 0xFFFFFFFFull) : (max_key >> 32);
            if ((half >> (shift & 31)) == 0) continue;
            VG_LAUNCH(vg::bm25u_radix_hist_kernel, dim3(static_cast<unsigned>(sort_chunks)), dim3(64), 0, st, key[cur], n_addp, shift, hist, sort_chunks);
            VG_LAUNCH(vg::prefix_kernel<uint32_t>, dim3(256), dim3(vg::kScanThreads), 0, st, hist, sort_chunks, digit_total, nullptr);
            VG_LAUNCH(vg::bm25u_radix_scatter_kernel, dim3(static_cast<unsigned>(sort_chunks)), dim3(64), 0, st, key[cur], tf[cur], n_addp, shift, hist,
                      digit_total, sort_chunks, key[cur ^ 1], tf[cur ^ 1]);
            cur ^= 1;
        }
    }
    {
        vg::ProfScope prof(ctx, "bm25_update_offsets", st);
        if (term_blocks)
            VG_LAUNCH(vg::bm25u_term_len_kernel, dim3(static_cast<unsigned>(term_blocks)), dim3(vg::kScanThreads), 0, st, bm->d_term_off, n_terms_old,
                      n_terms_new, lr, add_cnt, bm->d_alt_off, run_off, block_sum, term_blocks);
        VG_LAUNCH(vg::prefix_kernel<int64_t>, dim3(2), dim3(vg::kScanThreads), 0, st, block_sum, term_blocks, total, nullptr);
        VG_LAUNCH(vg::bm25u_term_fix_kernel, dim3(static_cast<unsigned>(n_terms_new / vg::kTermsPerBlock + 1)), dim3(vg::kScanThreads), 0, st,
                  bm->d_alt_off, run_off, n_terms_new, block_sum, term_blocks, total);
    }
    {
        vg::ProfScope prof(ctx, "bm25_update_merge", st);
        const vg::MergeArgs ma{bm->d_term_off, bm->d_post_doc, bm->d_post_tf, n_post,        n_terms_old,  lr,          bm->d_alt_off,
                               run_off,        key[cur],       tf[cur],       n_addp,        bm->d_alt_doc, bm->d_alt_tf, bm->alt_post_cap};
        if (chunks) VG_LAUNCH(vg::bm25u_merge_old_kernel, dim3(static_cast<unsigned>(chunks)), dim3(vg::kScanThreads), 0, st, ma);
        if (n_addp) VG_LAUNCH(vg::bm25u_merge_add_kernel, dim3(vg::grid_for(n_addp, 256)), dim3(256), 0, st, ma, err);
    }
    // the flag, the totals and the new offsets come back together: the call's one wait
    unsigned long long state[4] = {0, 0, 0, 0};
    std::vector<int64_t> h_off(static_cast<size_t>(n_terms_new) + 1);
    VG_HIP(hipMemcpyAsync(state, err, sizeof(state), hipMemcpyDeviceToHost, st));
    VG_HIP(hipMemcpyAsync(h_off.data(), bm->d_alt_off, h_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    VG_CHECK(state[0] != vg::kErrLiveSlot, VG_ERR_INVALID_ARG,
             "vg_bm25_update: added doc %llu still has a posting in a list it is added to (an add into a live slot: delete it in the same call)", state[1]);
    VG_CHECK(state[0] != vg::kErrDoc, VG_ERR_INVALID_ARG, "vg_bm25_update: a doc array in device memory names doc %llu, out of range", state[1]);
    VG_CHECK(state[0] != vg::kErrTerm, VG_ERR_INVALID_ARG, "vg_bm25_update: add_terms in device memory names term %llu, n_terms_new = %lld", state[1],
             (long long)n_terms_new);
    const int64_t n_post_new = static_cast<int64_t>(state[2]);
    VG_CHECK(n_post_new == h_off.back() && n_post_new <= n_post + n_addp, VG_ERR_HIP, "vg_bm25_update: the new offsets end at %lld, %lld postings counted",
             (long long)h_off.back(), (long long)n_post_new);

    // the checks have passed: the per-doc arrays (grown by capacity), deletes first, so that a replaced doc ends with its new length
    const bool want_ids = bm->mapped && n_docs_new > 0;
    if (n_docs_new > std::max(bm->docs_cap, n_docs_old) || (n_docs_new > 0 && !bm->d_doc_len) || (want_ids && !bm->d_doc_to_id)) {
        const int64_t have = std::max(bm->docs_cap, n_docs_old);
        const int64_t want = std::max(n_docs_new, have + have / 2);
        uint32_t *len = bm->d_doc_len, *ids = bm->d_doc_to_id;  // (a failed second growth leaves the first array larger than it need be, nothing else)
        VG_TRY(vg::grow_docs(&len, n_docs_old, want, st));
        bm->d_doc_len = len;
        if (want_ids) {
            VG_TRY(vg::grow_docs(&ids, n_docs_old, want, st));
            bm->d_doc_to_id = ids;
        }
        bm->docs_cap = want;
    }
    if (n_del) VG_LAUNCH(vg::bm25u_docs_del_kernel, dim3(vg::grid_for(n_del, 256)), dim3(256), 0, st, d_del.ptr, n_del, bm->d_doc_len, bm->d_doc_to_id);
    if (n_add)
        VG_LAUNCH(vg::bm25u_docs_add_kernel, dim3(vg::grid_for(n_add, 256)), dim3(256), 0, st, d_docs.ptr, d_len.ptr, d_ids.ptr, n_add, bm->d_doc_len,
                  bm->d_doc_to_id);
    std::swap(bm->d_post_doc, bm->d_alt_doc);
    std::swap(bm->d_post_tf, bm->d_alt_tf);
    std::swap(bm->d_term_off, bm->d_alt_off);
    const int64_t old_post_room = std::max(bm->post_cap, n_post), old_off_room = std::max(bm->off_cap, n_terms_old + 1);
    bm->post_cap = bm->alt_post_cap;
    bm->off_cap = bm->alt_off_cap;
    bm->alt_post_cap = bm->d_alt_doc ? old_post_room : 0;
    bm->alt_off_cap = old_off_room;
    bm->n_docs = n_docs_new;
    bm->n_terms = n_terms_new;
    bm->n_post = n_post_new;
    bm->h_term_off = std::move(h_off);
    vg::bm25_set_constants(bm, total_length, doc_count);
    return VG_OK;
}

VG_API int32_t vg_bm25_export(vg_bm25 *bm, int64_t *term_off, uint32_t *post_doc, uint32_t *post_tf, uint32_t *doc_len, uint32_t *doc_to_id, void *stream)
{
    VG_CHECK(bm, VG_ERR_INVALID_ARG, "vg_bm25_export: NULL index");
    VG_CHECK(!doc_to_id || bm->mapped, VG_ERR_INVALID_ARG, "vg_bm25_export: doc_to_id of an index that reports doc ids themselves");
    VG_HIP(hipSetDevice(bm->ctx->device));
    hipStream_t st = vg::pick_stream(bm->ctx, stream);
    bool host = false;
    auto copy = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        if (!dst || bytes == 0) return hipSuccess;
        const bool dev = vg::is_device_ptr(dst);
        host |= !dev;
        return hipMemcpyAsync(dst, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
    };
    VG_HIP(copy(term_off, bm->d_term_off, static_cast<size_t>(bm->n_terms + 1) * 8));
    VG_HIP(copy(post_doc, bm->d_post_doc, static_cast<size_t>(bm->n_post) * 4));
    VG_HIP(copy(post_tf, bm->d_post_tf, static_cast<size_t>(bm->n_post) * 4));
    VG_HIP(copy(doc_len, bm->d_doc_len, static_cast<size_t>(bm->n_docs) * 4));
    VG_HIP(copy(doc_to_id, bm->d_doc_to_id, static_cast<size_t>(bm->n_docs) * 4));
    if (host) VG_HIP(hipStreamSynchronize(st));
    return VG_OK;
}
