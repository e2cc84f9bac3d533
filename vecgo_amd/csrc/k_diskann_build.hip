// k_diskann_build.hip — diskann.Writer.Write (internal/segment/diskann/writer.go:217-272) on a resident index.
//   vg_diskann_build          the writer's steps 1, 2 and 2.5 in its order: quantize the rows in add order (:229-242, :274-360),
//                             buildGraph = vg_vamana_build, reorderBFS = vg_vamana_reorder_bfs.  Every refusal of those calls is
//                             made first, so that a refusal leaves neither codes nor a graph behind.
//   vg_segment_write_diskann  step 3, Flush (:645-856): the 160-byte header (format.go:51-78), then with no padding between them
//                             the fp32 rows, the graph, the codes and their parameters, the ids, the two metadata sections; the
//                             body's CRC-32C computed on the device (vg_crc_device.hpp) for the rows, the graph and the codes.
// Host code only: the kernels are those of the calls it makes and the CRC kernels of k_flat_build.hip.
#include <vector>

#include "vg_crc32c.hpp"
#include "vg_crc_device.hpp"
#include "vg_internal.hpp"
#include "vg_search.hpp"
#include "vg_segment_layout.hpp"

namespace vg {

// ---- the image's layout (writer.go:645-833) -----------------------------------------------------------------------------
struct DiskImage {
    int qtype = VG_QUANT_NONE;                                                           // quantization.Type of the codes on the index
    uint64_t vectors = 0, graph = 0, codes = 0, params = 0, pk = 0, metadata = 0, md_index = 0;  // section bytes
    uint64_t total() const { return seglayout::kDiskHeader + vectors + graph + codes + params + pk + metadata + md_index; }
};

// the sections' sizes, and what about the index the writer refuses; metadata_bytes / index_bytes < 0: what the writer emits when
// no row has a document
static int32_t disk_image_plan(const vg_index *idx, int64_t metadata_bytes, int64_t index_bytes, DiskImage &L, const char *fn)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(idx->n > 0, VG_ERR_INVALID_ARG, "%s: no vectors to write", fn);  // writer.go:218-220
    VG_CHECK(idx->d_vectors, VG_ERR_NOT_READY, "%s: index has no fp32 rows", fn);
    VG_CHECK(idx->d_vamana && idx->vamana_r > 0, VG_ERR_NOT_READY, "%s: index has no Vamana graph", fn);
    VG_CHECK(!idx->d_hnsw_l0 && !idx->d_centroids && idx->num_partitions == 0 && !idx->d_sq_tiles, VG_ERR_UNSUPPORTED,
             "%s: the index holds %s, which a DiskANN segment never has", fn,
             idx->d_hnsw_l0 ? "an HNSW graph" : idx->d_sq_tiles ? "SQ8 codes" : "IVF partitions");
    const bool pq = idx->pq && idx->d_pq_rows, rq = idx->d_rq_rows != nullptr, i4 = idx->d_int4_rows != nullptr;
    VG_CHECK(int(pq) + int(rq) + int(i4) <= 1, VG_ERR_UNSUPPORTED, "%s: the index holds more than one kind of codes, a DiskANN segment has one",
             fn);
    VG_CHECK(idx->n <= 0xFFFFFFFFll, VG_ERR_UNSUPPORTED, "%s: RowCount is a uint32", fn);
    VG_CHECK(!pq || (idx->pq->m <= 0xFFFF && idx->pq->k <= 0xFFFF), VG_ERR_UNSUPPORTED, "%s: PQSubvectors and PQCentroids are uint16", fn);
    const uint64_t n = static_cast<uint64_t>(idx->n), dim = static_cast<uint64_t>(idx->dim);
    L.qtype = pq ? VG_QUANT_PQ : rq ? VG_QUANT_RABITQ : i4 ? VG_QUANT_INT4 : VG_QUANT_NONE;
    L.vectors = n * dim * 4;
    L.graph = n * static_cast<uint64_t>(idx->vamana_r) * 4;
    if (pq) {  // :742-763: scales, offsets, codebooks — no (m, K) in front, unlike the flat format
        const uint64_t m = static_cast<uint64_t>(idx->pq->m);
        L.codes = n * m;
        L.params = m * 8 + m * static_cast<uint64_t>(idx->pq->k) * idx->pq->subdim;
    } else if (rq) {
        L.codes = n * seglayout::rabitq_code_bytes(dim);
    } else if (i4) {  // :764-775 Int4Quantizer.MarshalBinary (quantization/int4.go:171-188): u32 dim, min[dim], diff[dim]
        L.codes = n * ((dim + 1) / 2);
        L.params = 4 + dim * 8;
    }
    L.pk = n * 8;
    L.metadata = metadata_bytes >= 0 ? static_cast<uint64_t>(metadata_bytes) : (n + 1) * 8;  // :797-823 with every md nil
    L.md_index = index_bytes >= 0 ? static_cast<uint64_t>(index_bytes) : 1;                 // unified.go:1724-1733, empty index
    return VG_OK;
}

}  // namespace vg

VG_API int32_t vg_diskann_build(vg_index *idx, int32_t r, int32_t l, float alpha, int32_t quantization, int32_t pq_m, int32_t pq_iters,
                                uint64_t seed, int32_t max_batch, int32_t growth_div, vg_pq *pq, vg_int4 *iq, uint32_t *perm,
                                uint32_t *inv_perm, int32_t *quantization_used, void *stream)
{
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "vg_diskann_build: NULL index");
    VG_CHECK(idx->n == 0 || idx->d_vectors, VG_ERR_NOT_READY, "vg_diskann_build: index has no fp32 rows");
    VG_CHECK(idx->n > 0, VG_ERR_INVALID_ARG, "vg_diskann_build: no vectors to write");  // writer.go:218-220
    const char *held = vg::held_segment_state(idx);
    if (!held) held = idx->d_hnsw_l0 ? "an HNSW graph" : idx->d_hnsw_tomb ? "HNSW tombstones" : idx->d_hnsw_l0_dist ? "HNSW edge distances" : nullptr;
    VG_CHECK(!held, VG_ERR_UNSUPPORTED, "vg_diskann_build: the index holds %s: the writer quantizes, builds and reorders bare rows", held);
    VG_CHECK(quantization == VG_QUANT_NONE || quantization == VG_QUANT_PQ || quantization == VG_QUANT_RABITQ || quantization == VG_QUANT_INT4,
             VG_ERR_INVALID_ARG, "vg_diskann_build: quantization %d is none of VG_QUANT_NONE / _PQ / _RABITQ / _INT4 (writer.go:229-242)",
             quantization);
    VG_CHECK(quantization != VG_QUANT_PQ || pq, VG_ERR_INVALID_ARG, "vg_diskann_build: VG_QUANT_PQ without a vg_pq");
    VG_CHECK(quantization != VG_QUANT_INT4 || iq, VG_ERR_INVALID_ARG, "vg_diskann_build: VG_QUANT_INT4 without a vg_int4");
    if (quantization == VG_QUANT_PQ) {
        // (the reference skips training then, writer.go:230, and still writes a header that claims PQ, :678-681)
        VG_CHECK(pq_m > 0, VG_ERR_INVALID_ARG, "vg_diskann_build: VG_QUANT_PQ with pq_m = %d", pq_m);
        VG_CHECK(pq->m == pq_m && pq->k == 256, VG_ERR_INVALID_ARG,
                 "vg_diskann_build: the vg_pq has m = %d, k = %d; the writer's is NewProductQuantizer(dim, %d, 256) (writer.go:281-285)", pq->m,
                 pq->k, pq_m);
        VG_CHECK(pq->dim == idx->dim, VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
    }
    if (quantization == VG_QUANT_INT4) VG_CHECK(iq->dim == idx->dim, VG_ERR_DIM_MISMATCH, "dimension mismatch");
    const int64_t n = idx->n;
    const bool train_pq = quantization == VG_QUANT_PQ && n >= 256;  // trainPQ (:276-279): fewer rows than centroids switch PQ off
    if (train_pq) {
        VG_CHECK(pq_iters >= 0, VG_ERR_INVALID_ARG, "vg_pq_train: iters < 0");
        VG_TRY(vg::pq_train_refusal(pq, n));
    }
    if (quantization == VG_QUANT_RABITQ)
        VG_CHECK(idx->dim <= 8192, VG_ERR_UNSUPPORTED, "vg_index_set_rabitq_codes: dim %d > 8192", idx->dim);
    VG_TRY(vg::vamana_build_check(idx, r, l, alpha, max_batch, growth_div));

    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    int32_t used = VG_QUANT_NONE;
    // 1. the quantizer and the codes, over the rows in add order
    if (train_pq) {
        vg::DevTmp<uint8_t> codes;
        VG_TRY(codes.init(static_cast<size_t>(n) * pq->m, st));
        VG_TRY(vg_pq_train(pq, idx->d_vectors, n, pq_iters ? pq_iters : 20, seed, stream));
        VG_TRY(vg_pq_encode(pq, idx->d_vectors, n, codes.ptr, stream));
        VG_TRY(vg_index_set_pq_codes(idx, pq, codes.ptr, stream));
        used = VG_QUANT_PQ;
    } else if (quantization == VG_QUANT_RABITQ) {
        vg::DevTmp<uint8_t> codes;
        VG_TRY(codes.init(static_cast<size_t>(n) * static_cast<size_t>(vg_rabitq_code_bytes(idx->dim)), st));
        VG_TRY(vg_rabitq_encode(idx->ctx, idx->dim, idx->d_vectors, n, codes.ptr, stream));
        VG_TRY(vg_index_set_rabitq_codes(idx, codes.ptr, stream));
        used = VG_QUANT_RABITQ;
    } else if (quantization == VG_QUANT_INT4) {
        vg::DevTmp<uint8_t> codes;
        VG_TRY(codes.init(static_cast<size_t>(n) * static_cast<size_t>(vg_int4_code_bytes(idx->dim)), st));
        VG_TRY(vg_int4_train(iq, idx->d_vectors, n, stream));
        VG_TRY(vg_int4_encode(iq, idx->d_vectors, n, codes.ptr, stream));
        VG_TRY(vg_index_set_int4_codes(idx, iq, codes.ptr, stream));
        used = VG_QUANT_INT4;
    }
    // 2. the graph, 2.5 its BFS order: the codes move with the rows
    VG_TRY(vg_vamana_build(idx, r, l, alpha, nullptr, seed, max_batch, growth_div, stream));
    VG_TRY(vg_vamana_reorder_bfs(idx, perm, inv_perm, stream));
    if (quantization_used) *quantization_used = used;
    return VG_OK;
}

VG_API int64_t vg_segment_diskann_image_size(const vg_index *idx, int64_t metadata_bytes, int64_t metadata_index_bytes)
{
    vg::DiskImage L;
    if (vg::disk_image_plan(idx, metadata_bytes, metadata_index_bytes, L, "vg_segment_diskann_image_size") != VG_OK) return -1;
    return static_cast<int64_t>(L.total());
}

VG_API int32_t vg_segment_write_diskann(vg_index *idx, uint64_t segment_id, int32_t search_list_size, int32_t compression_type,
                                        const uint64_t *ids, const void *metadata_section, int64_t metadata_bytes,
                                        const void *metadata_index, int64_t metadata_index_bytes, void *image, int64_t image_size,
                                        int64_t *written, void *stream)
{
    using namespace vg::seglayout;
    const char *fn = "vg_segment_write_diskann";
    if (written) *written = 0;
    VG_CHECK(idx, VG_ERR_INVALID_ARG, "%s: NULL index", fn);
    VG_CHECK(image, VG_ERR_INVALID_ARG, "%s: image is NULL", fn);
    VG_CHECK(compression_type >= 0 && compression_type <= 2, VG_ERR_INVALID_ARG, "%s: compression_type %d is none of 0, 1, 2", fn,
             compression_type);
    VG_CHECK(search_list_size >= 0, VG_ERR_INVALID_ARG, "%s: search_list_size %d is negative", fn, search_list_size);
    VG_CHECK((!metadata_section || metadata_bytes >= 0) && (!metadata_index || metadata_index_bytes >= 0), VG_ERR_INVALID_ARG,
             "%s: negative section size", fn);
    vg::DiskImage L;
    VG_TRY(vg::disk_image_plan(idx, metadata_section ? metadata_bytes : -1, metadata_index ? metadata_index_bytes : -1, L, fn));
    VG_CHECK(image_size >= 0 && static_cast<uint64_t>(image_size) >= L.total(), VG_ERR_INVALID_ARG,
             "%s: the image needs %llu bytes, the buffer has %lld", fn, static_cast<unsigned long long>(L.total()),
             static_cast<long long>(image_size));
    VG_HIP(hipSetDevice(idx->ctx->device));
    hipStream_t st = vg::pick_stream(idx->ctx, stream);
    const int64_t n = idx->n;
    const int32_t dim = idx->dim;
    uint8_t *img = static_cast<uint8_t *>(image);
    // writer.go:695-833: bytesWritten, a running sum
    const uint64_t o_vec = kDiskHeader, o_graph = o_vec + L.vectors, o_codes = o_graph + L.graph, o_params = o_codes + L.codes,
                   o_pk = o_params + L.params, o_meta = o_pk + L.pk, o_index = o_meta + L.metadata;
    const uint8_t *d_codes = L.qtype == VG_QUANT_PQ ? idx->d_pq_rows : L.qtype == VG_QUANT_RABITQ ? idx->d_rq_rows : idx->d_int4_rows;

    // the device's share of the checksum: rows, graph and codes, virtually every byte of the body
    const vg::CrcTables *tables = nullptr;
    VG_TRY(vg::crc_tables(idx->ctx->device, &tables));
    vg::CrcJob job_rows, job_graph, job_codes;
    job_rows.plan(idx->d_vectors, static_cast<int64_t>(L.vectors));
    job_graph.plan(idx->d_vamana, static_cast<int64_t>(L.graph));
    job_codes.plan(d_codes, static_cast<int64_t>(L.codes));
    vg::DevTmp<uint32_t> d_crc;
    VG_TRY(d_crc.init(job_rows.words() + job_graph.words() + job_codes.words(), st));
    uint32_t *d_crc_graph = d_crc.ptr + job_rows.words(), *d_crc_codes = d_crc_graph + job_graph.words();
    {
        vg::ProfScope prof(idx->ctx, "crc32c_device", st);
        VG_TRY(job_rows.launch(idx->d_vectors, tables, d_crc.ptr, st));
        VG_TRY(job_graph.launch(idx->d_vamana, tables, d_crc_graph, st));
        if (L.codes) VG_TRY(job_codes.launch(d_codes, tables, d_crc_codes, st));
    }
    // the quantizer's parameters, then the host's own sections, while those kernels run
    if (L.qtype == VG_QUANT_PQ) {
        const uint64_t m = static_cast<uint64_t>(idx->pq->m);
        VG_HIP(hipMemcpyAsync(img + o_params, idx->pq->d_scales, m * 4, hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(img + o_params + m * 4, idx->pq->d_offsets, m * 4, hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(img + o_params + m * 8, idx->pq->d_codebooks, L.params - m * 8, hipMemcpyDeviceToHost, st));
    } else if (L.qtype == VG_QUANT_INT4) {
        wr32(img + o_params, static_cast<uint32_t>(dim));
        VG_HIP(hipMemcpyAsync(img + o_params + 4, idx->int4_min, static_cast<size_t>(dim) * 4, hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(img + o_params + 4 + static_cast<size_t>(dim) * 4, idx->int4_diff, static_cast<size_t>(dim) * 4,
                              hipMemcpyDeviceToHost, st));
    }
    for (int64_t i = 0; i < n; i++) wr64(img + o_pk + 8 * static_cast<uint64_t>(i), ids ? ids[i] : static_cast<uint64_t>(i));
    if (metadata_section) {
        if (L.metadata) memcpy(img + o_meta, metadata_section, L.metadata);
    } else {
        memset(img + o_meta, 0, L.metadata);  // rows + 1 zero uint64 offsets, no blob
    }
    if (metadata_index) {
        if (L.md_index) memcpy(img + o_index, metadata_index, L.md_index);
    } else {
        img[o_index] = 0;  // WriteInvertedIndex of an empty index
    }
    std::vector<uint32_t> h_crc(job_rows.words() + job_graph.words() + job_codes.words());
    VG_HIP(hipMemcpyAsync(h_crc.data(), d_crc.ptr, h_crc.size() * 4, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));  // the parameters are in the image, the registers on the host
    // the big sections go home while the host checksums its own
    VG_HIP(hipMemcpyAsync(img + o_vec, idx->d_vectors, L.vectors, hipMemcpyDeviceToHost, st));
    VG_HIP(hipMemcpyAsync(img + o_graph, idx->d_vamana, L.graph, hipMemcpyDeviceToHost, st));
    if (L.codes) VG_HIP(hipMemcpyAsync(img + o_codes, d_codes, L.codes, hipMemcpyDeviceToHost, st));
    uint32_t crc = vg::crc::finish_raw(job_rows.finish(h_crc.data()), L.vectors);
    crc = vg::crc::combine(crc, vg::crc::finish_raw(job_graph.finish(h_crc.data() + job_rows.words()), L.graph), L.graph);
    if (L.codes)
        crc = vg::crc::combine(crc, vg::crc::finish_raw(job_codes.finish(h_crc.data() + job_rows.words() + job_graph.words()), L.codes), L.codes);
    const uint64_t rest = L.total() - o_params;
    crc = vg::crc::combine(crc, vg_crc32c(img + o_params, static_cast<int64_t>(rest)), rest);
    // the header (format.go:51-78); an absent section's offset stays 0 (writer.go:727-775), BlockStatsOffset is never set
    memset(img, 0, kDiskHeader);
    wr32(img, kDiskMagic);
    wr32(img + 4, 2);
    wr64(img + 8, segment_id);
    wr32(img + 16, static_cast<uint32_t>(n));
    wr32(img + 20, static_cast<uint32_t>(dim));
    img[24] = static_cast<uint8_t>(idx->metric);
    wr32(img + 25, static_cast<uint32_t>(idx->vamana_r));
    wr32(img + 29, static_cast<uint32_t>(search_list_size ? search_list_size : 100));  // NewWriter's default L (writer.go:102-104)
    wr32(img + 33, idx->vamana_entry);
    img[37] = static_cast<uint8_t>(L.qtype);
    if (L.qtype == VG_QUANT_PQ) {
        wr16(img + 38, static_cast<uint16_t>(idx->pq->m));
        wr16(img + 40, static_cast<uint16_t>(idx->pq->k));
    }
    img[42] = static_cast<uint8_t>(compression_type);
    wr64(img + 48, o_vec);
    wr64(img + 56, o_graph);
    if (L.qtype == VG_QUANT_PQ || L.qtype == VG_QUANT_INT4) wr64(img + 64, o_codes);
    if (L.qtype == VG_QUANT_RABITQ) wr64(img + 72, o_codes);
    if (L.params) wr64(img + 80, o_params);
    wr64(img + 88, o_pk);
    wr64(img + 96, o_meta);
    wr64(img + 112, o_index);
    wr32(img + 120, crc);
    VG_HIP(hipStreamSynchronize(st));
    if (written) *written = static_cast<int64_t>(L.total());
    return VG_OK;
}
