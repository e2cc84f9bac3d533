// vg_bm25.hpp — the resident BM25 index as its two translation units see it: k_bm25.hip (create, search, fusion) and
// k_bm25_update.hip (create_empty, update, export).
#pragma once

#include <vector>

#include "vg_internal.hpp"

struct vg_bm25 {
    vg_ctx *ctx = nullptr;
    int64_t n_docs = 0, n_terms = 0, n_post = 0;
    int64_t doc_count = 0;           // idx.docCount as the caller last gave it: 0 = an index that answers nothing (bm25.go:286)
    int64_t *d_term_off = nullptr;   // n_terms + 1
    uint32_t *d_post_doc = nullptr;  // n_post, ascending inside a term's list
    uint32_t *d_post_tf = nullptr;   // n_post
    uint32_t *d_doc_len = nullptr;   // n_docs
    uint32_t *d_doc_to_id = nullptr; // n_docs, or null: identity
    bool mapped = false;             // reports through doc_to_id (an empty mapped index has no array yet)
    // vg_bm25_update builds the next image beside the current one: the other half of each ping-pong pair, and the room each
    // array has (elements; 0 = exactly what it holds, as vg_bm25_create allocates)
    int64_t *d_alt_off = nullptr;
    uint32_t *d_alt_doc = nullptr, *d_alt_tf = nullptr;
    int64_t off_cap = 0, alt_off_cap = 0, post_cap = 0, alt_post_cap = 0, docs_cap = 0;
    unsigned long long *d_replayed = nullptr;  // [1] queries the heap replay answered
    std::vector<int64_t> h_term_off;           // the offsets on the host: the lists' lengths bound a query's hits
    double k1_plus_1 = 0, k1_1b = 0, k1_b_avgdl = 0;  // bm25.go:314-317
};

namespace vg {

// the three constants of bm25.go:314-317 from the caller's totals, and doc_count itself (k_bm25.hip: one place forms them, for
// vg_bm25_create and vg_bm25_update alike)
void bm25_set_constants(vg_bm25 *bm, int64_t total_length, int64_t doc_count);

// `count` elements of a caller's array on the host: where they lie, or copied back on the stream (which is then waited for)
template <typename T>
int32_t host_view(const T *p, size_t count, hipStream_t st, std::vector<T> &store, const T *&out)
{
    out = p;
    if (count == 0 || !is_device_ptr(p)) return VG_OK;
    store.resize(count);
    VG_HIP(hipMemcpyAsync(store.data(), p, count * sizeof(T), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    out = store.data();
    return VG_OK;
}

}  // namespace vg
