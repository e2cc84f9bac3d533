/*
 * vecgo_hip.h — C ABI of libvecgo_hip.so: the MI355X (gfx950) implementation of
 * vecgo's distance + quantization hot path.
 *
 * This is the drop-in boundary.  Every entry point names the reference interface
 * (file:line under the vecgo repository root) it stands in for.  Plain C types,
 * caller-owned buffers, no callbacks; INTEGRATION.md shows the cgo binding a
 * vecgo maintainer would add (internal/simd/kernels_hip.go + quantization shims).
 *
 * Conventions
 *   - Every function returns a vg_status (0 = ok, negative = error) and never
 *     aborts; vg_last_error() gives the message for the calling thread.
 *   - Data pointers may be HOST or DEVICE (HBM) pointers; the library detects
 *     which (hipPointerGetAttributes).  Host buffers are staged through HBM and
 *     the call returns after the results are back in the caller's buffer (the Go
 *     `//go:noescape` contract: no pointer is retained).  When every buffer of a
 *     call is a device pointer, all of the call's work is enqueued on `stream`, in
 *     order with what the caller enqueued there before; results are ready when the
 *     stream reaches that point.  Whether the call also returns before that work
 *     has run depends on the entry point: see "Enqueue-only entry points" below.
 *   - Alignment: a pointer must be aligned to its element type (4 bytes for float,
 *     uint32_t and int32_t; 1 for codes and masks) and to nothing more.  ANY
 *     ELEMENT-ALIGNED DEVICE POINTER IS ACCEPTED AND GIVES THE SAME BITS as a 16-byte
 *     aligned one — a row range of a larger tensor, a slice of an arena.  Where a
 *     kernel needs 16-byte aligned operands the library either runs its element-wise
 *     twin or passes the buffer through a scratch block with device-to-device copies on
 *     `stream` (nothing waits); a 16-byte aligned device pointer is always used where it
 *     lies, which is the fast path.  Host pointers are staged whatever their alignment.
 *   - Enqueue-only entry points.  With every buffer device-resident these return as
 *     soon as their work is enqueued, without waiting for `stream`: vg_sq8_encode /
 *     _decode / _l2_distance_batch, vg_int4_encode / _decode / _l2_distance_batch,
 *     vg_pq_encode / _decode / _asymmetric_distance_batch / _build_distance_table,
 *     vg_pq_adc_lookup_batch, vg_opq_rotate / _encode / _decode /
 *     _asymmetric_distance_batch, vg_binary_encode / _decode / _hamming_batch,
 *     vg_normalize_l2, vg_rabitq_encode / _distance_batch, vg_kmeans_assign,
 *     vg_search_flat, vg_search_flat_threshold (batches below its nomination),
 *     vg_search_flat_probed_threshold, vg_search_flat_filtered, vg_search_flat_probed, vg_search_sq8 and vg_search_pq_adc
 *     (batches that keep the scan), vg_search_rabitq, vg_search_hnsw, vg_search_hnsw_pq,
 *     vg_search_hnsw_filtered, vg_search_hnsw_predicate, vg_search_vamana (k <= 512),
 *     vg_search_vamana_filtered, vg_search_vamana_threshold, vg_rerank,
 *     vg_score_candidates, vg_filter_evaluate, vg_mask_combine, vg_mask_popcount, vg_mask_to_rows, vg_rrf_fuse — with stats == NULL where there is one.  (The first call of
 *     an entry on a stream may allocate its scratch; tests/test_gpu_device_buffers.py
 *     asserts the list.)
 *     These WAIT for `stream` inside the call, device buffers or not, because the host
 *     needs a value the device computes: every *_train (the solves and convergence tests
 *     are the host's); the builders and maintenance calls (vg_hnsw_build / _insert /
 *     _compact, vg_vamana_build, vg_vamana_insert, vg_vamana_consolidate, vg_vamana_reorder_bfs, vg_flat_build, vg_diskann_build,
 *     vg_index_merge, vg_segment_*); vg_index_set_* and vg_index_enable_* (storage is replaced; the
 *     caller's buffer is free again at return); every getter; vg_search_hnsw_brute (reads
 *     its filter's population count and redo flags back); vg_search_flat_prefilter (reads its
 *     masks' population counts back to size its row lists); vg_bm25_create (like vg_index_set_*) and
 *     vg_bm25_search (query term arrays in device memory are read back: the terms' list lengths size the
 *     key lists); vg_bm25_update (reads its error flag and the new offsets back) and vg_bm25_export to host memory; vg_search_sq8 and
 *     vg_search_pq_adc when the bfloat16 nomination takes the batch, and
 *     vg_search_flat_threshold when its nomination does (the proofs' flags are read
 *     back); any call that is handed a host buffer, a stats array on the host included.
 *     Entry points in neither list make no promise either way.
 *   - `stream` is a hipStream_t passed as void*.  NULL = the context's own (non-blocking)
 *     stream — right for host-buffer callers such as cgo.  A caller that produces device
 *     buffers on HIP's legacy default stream (handle 0, e.g. PyTorch's default stream) must
 *     pass VG_STREAM_LEGACY so that its work and the library's are ordered.
 *   - Index / quantizer handles may be used from many threads at once for the
 *     read-only calls (search, encode, build table); create / set / train /
 *     destroy must be externally serialised (internal/quantization/doc.go:120-123).
 *   - Zero-length inputs succeed and produce empty / zero outputs
 *     (internal/simd/kernels_amd64.go:291-297).
 *   - Result ids are uint32 row ids (model.RowID); unused result slots hold
 *     id 0xFFFFFFFF and score +Inf (L2-like) or -Inf (Dot).
 */
#ifndef VECGO_HIP_H
#define VECGO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct the caller allocates, or an entry point's argument list, changes; vg_abi_version()
 * returns the value the library was built with — a host compares the two before its first call.
 *   2: vg_search_stats has FIVE int64 (descent_distance_computations was appended): vg_search_hnsw / _hnsw_pq /
 *      _vamana write nq * 5 values. */
#define VG_ABI_VERSION 2
/* Bumped whenever entry points are ADDED (nothing existing changes): a binding that wants a newer entry point compares
 * vg_abi_minor() with the value below before it looks the symbol up, instead of failing on first use.
 *   1: (r04) vg_search_hnsw_brute, vg_debug_heap_replay
 *   2: (r05) vg_abi_minor itself; no other symbol added — vg_search_hnsw / _hnsw_pq answer NaN distances as the reference
 *      does, vg_kmeans_* decide assignments on the matrix cores, the k-means++ running sum of vg_pq_train is blocked
 *   3: (r05) vg_search_hnsw_filtered
 *   4: (r05) vg_search_flat_filtered
 *   5: (r05) vg_search_vamana_filtered
 *   6: (r05) vg_search_hnsw_predicate, vg_index_set_hnsw_edge_distances; vg_search_hnsw_filtered serves every selectivity
 *   7: (r05) vg_index_set_hnsw_tombstones
 *   8: (r05) vg_segment_search_filtered
 *   9: (r05) vg_index_enable_sq8_nomination
 *  10: (r06) vg_index_enable_pq_nomination; NaN scores answered as the reference's heaps answer them (see "NaN scores")
 *  11: vg_search_flat_threshold
 *  12: vg_vamana_build, vg_index_get_vamana_graph
 *  13: vg_hnsw_insert
 *  Added at minor 13 without a bump (the minor-13 header test pins the value): vg_search_vamana_threshold,
 *  vg_vamana_reorder_bfs, and vg_search_vamana / _filtered take k up to 16384 (512 before).  A binding that needs
 *  them looks the symbol vg_search_vamana_threshold up (dlsym) instead of comparing the minor, and
 *  vg_vamana_reorder_bfs the same way; the next bump covers them.  Likewise the flat writer: vg_flat_build,
 *  vg_segment_flat_image_size, vg_segment_write_flat and vg_crc32c_device — bindings find them by symbol lookup.
 *  Likewise vg_hnsw_compact (with its caller-allocated vg_hnsw_compact_stats).  Likewise the DiskANN writer:
 *  vg_diskann_build, vg_segment_diskann_image_size and vg_segment_write_diskann, found by symbol lookup.  Likewise the
 *  threshold search over coded / partitioned flat segments: vg_search_flat_probed_threshold and
 *  vg_segment_search_threshold, found by symbol lookup.  Likewise the streaming Vamana index: vg_vamana_insert and
 *  vg_search_vamana_fresh, found by symbol lookup; and its delete path, vg_vamana_consolidate (with its caller-allocated
 *  vg_vamana_consolidate_stats), the same way.  Likewise vg_index_flat_retried and
 *  vg_index_flat_appended, found by symbol lookup.  Likewise the compaction's merge of resident indexes under tombstones,
 *  vg_index_merge, found by symbol lookup.  Likewise the metadata filters evaluated on the device: vg_columns_create /
 *  _destroy / _set_f64 / _set_codes / _drop, vg_filter_evaluate (with its caller-allocated vg_filter_clause),
 *  vg_mask_combine, vg_mask_popcount and vg_mask_alloc / _free, found by symbol lookup.  Likewise the pre-filter search
 *  (the engine's bitmap strategy): vg_mask_to_rows and vg_search_flat_prefilter, found by symbol lookup.  Likewise hybrid
 *  search (the lexical leg and the fusion of Engine.HybridSearch): vg_bm25_create / _destroy / _stats / _search / _replayed and
 *  vg_rrf_fuse, found by symbol lookup.  Likewise the writes to a resident BM25 index: vg_bm25_create_empty, vg_bm25_update
 *  and vg_bm25_export, found by symbol lookup.  Likewise the PQ batch nomination from the codes:
 *  vg_index_enable_pq_nomination_from_codes and vg_index_pq_nomination_info, found by symbol lookup.  Likewise the SQ8 batch
 *  nomination from the codes: vg_index_enable_sq8_nomination_from_codes and vg_index_sq8_nomination_info, found by symbol lookup.  Likewise the test
 *  entry point vg_int4_scan_plan, found by symbol lookup.  Likewise the RaBitQ batch nomination on the int8 matrix cores:
 *  vg_index_enable_rabitq_nomination and vg_index_rabitq_nomination_info, found by symbol lookup.  Likewise the exhaustive
 *  search over an index's INT4 codes, vg_search_int4, found by symbol lookup. */
#define VG_ABI_MINOR 13
#define VG_INVALID_ID 0xFFFFFFFFu
#define VG_STREAM_LEGACY ((void *)1) /* == hipStreamLegacy */

/* error conventions: Go (value, error) strings in parentheses are what the Go
 * shim maps each code to (internal/quantization/pq.go:148-153,190,496;
 * rabitq.go:53,124) */
typedef enum vg_status {
    VG_OK = 0,
    VG_ERR_INVALID_ARG = -1,        /* nil/negative/inconsistent arguments */
    VG_ERR_DIM_MISMATCH = -2,       /* "vector dimension mismatch" */
    VG_ERR_NOT_TRAINED = -3,        /* "ProductQuantizer not trained" */
    VG_ERR_CODE_LENGTH = -4,        /* "codes length mismatch" / "invalid code length" */
    VG_ERR_UNSUPPORTED = -5,        /* "unsupported metric for float32: ..." / shape not supported */
    VG_ERR_OUT_OF_MEMORY = -6,
    VG_ERR_HIP = -7,                /* a HIP runtime call failed */
    VG_ERR_NO_DEVICE = -8,          /* no gfx950 device / extension not usable */
    VG_ERR_NOT_READY = -9,          /* index lacks the data this search needs */
    VG_ERR_FORMAT = -10,            /* segment image: "invalid magic number", "file too short for ..." */
    VG_ERR_CHECKSUM = -11           /* segment image: "checksum mismatch: expected %x, got %x" */
} vg_status;

/* distance.Metric — distance/distance.go:66-73 */
typedef enum vg_metric {
    VG_METRIC_L2 = 0,
    VG_METRIC_COSINE = 1,
    VG_METRIC_DOT = 2,
    VG_METRIC_HAMMING = 3
} vg_metric;

typedef struct vg_ctx vg_ctx;     /* one per (process, GPU) */
typedef struct vg_pq vg_pq;       /* quantization.ProductQuantizer — pq.go:20-29 */
typedef struct vg_index vg_index; /* device-resident rows / codes / graph of one segment */
typedef struct vg_sq8 vg_sq8;     /* quantization.ScalarQuantizer — quantizer.go:27-39 */
typedef struct vg_int4 vg_int4;   /* quantization.Int4Quantizer — int4.go:12-20 */
typedef struct vg_segment vg_segment; /* an opened flat / DiskANN segment image: index + quantizers */

/* ---- context ------------------------------------------------------------ */
int32_t vg_abi_version(void);
int32_t vg_abi_minor(void);
/* device = HIP ordinal (LOCAL_RANK in a one-process-per-GPU job) */
int32_t vg_ctx_create(int32_t device, vg_ctx **out);
int32_t vg_ctx_destroy(vg_ctx *ctx);
int32_t vg_ctx_synchronize(vg_ctx *ctx, void *stream);
const char *vg_last_error(void);
const char *vg_status_string(int32_t status);
/* name (e.g. "gfx950"), CU count and HBM bytes of the context's device */
int32_t vg_ctx_device_info(vg_ctx *ctx, char *arch, int32_t arch_len, int32_t *compute_units,
                           int64_t *hbm_bytes);

/* per-kernel timing with HIP events on the launching stream (the analogue of the reference's
 * per-query FilterGateStats.SearchTimeNanos, searcher/searcher.go:114-137).  While enabled,
 * every launch of the named hot kernels is bracketed by an event pair.  vg_profile_read
 * synchronises, then returns the number of launches and their summed duration since the last
 * read for `kernel` ("flat_gemm", "flat_retry", "pq_adc_scan", "rabitq_scan", "flat_select", "topk_merge",
 * "hnsw_search", "vamana_search"), and clears those records.  The name "staged_device_buffers" is a counter, not a
 * kernel: how many misaligned DEVICE buffers the process passed through a scratch block since the last read ("Alignment"
 * above), profiling enabled or not; total_ms is 0.  Likewise "flat_split_launches": launches of vg_search_flat's split
 * nomination tile (three bfloat16 products on the fp32 rows) since the last read. */
int32_t vg_profile_enable(vg_ctx *ctx, int32_t on);
int32_t vg_profile_read(vg_ctx *ctx, const char *kernel, int64_t *launches, double *total_ms);

/* ---- ProductQuantizer (internal/quantization/pq.go) ------------------------ */
/* NewProductQuantizer pq.go:36-64: dim % m == 0, 0 < k <= 256 */
int32_t vg_pq_create(vg_ctx *ctx, int32_t dim, int32_t m, int32_t k, vg_pq **out);
int32_t vg_pq_destroy(vg_pq *pq);
/* SetCodebooks pq.go:458-464: int8 codebooks m*k*(dim/m), scales[m], offsets[m] */
int32_t vg_pq_set_codebooks(vg_pq *pq, const int8_t *codebooks, const float *scales,
                            const float *offsets);
/* Codebooks pq.go:452-455 (copies out) */
int32_t vg_pq_get_codebooks(vg_pq *pq, int8_t *codebooks, float *scales, float *offsets);
int32_t vg_pq_is_trained(vg_pq *pq);
/* BuildDistanceTable pq.go:468-491, batched: tables[nq][m*k] (entry = a8 term,
 * internal/simd/kernels.go:354-374 generic order, no FMA) */
int32_t vg_pq_build_distance_table(vg_pq *pq, const float *queries, int64_t nq, float *tables,
                                   void *stream);

/* Train pq.go:68-143: per sub-quantizer k-means++ init + <= iters Lloyd iterations on fp32
 * sub-vectors, then int8 quantisation of the centroids (pq.go:97-136).  vectors[n*dim].
 * The reference draws from the unseeded global math/rand (pq.go:294,308,314,409), so trained
 * codebooks are not reproducible there; here every draw comes from a counter-based stream
 * keyed by `seed` (the CPU oracle uses the same stream, so GPU == oracle bit for bit).
 * The reference uses iters = 20.
 * STATED DEVIATION from the reference's arithmetic (not a restatement): the k-means++ seeding adds
 * minDistSq up — for the total and again for the pick — in blocks of 64 with a pairwise tree inside a
 * block and a sequential sum over the block totals, where pq.go:296-336 runs ONE fp32 accumulator over
 * all n values in index order.  For the same draw the picked row can therefore differ from the
 * reference's where the target lies within rounding distance of a prefix sum; the reference's own draws
 * are unseeded, so no trained codebook of it can be reproduced either way (trained
 * codebooks are quality-parity only).  The oracle implements the same blocked sum (oracle/vg_oracle.c). */
int32_t vg_pq_train(vg_pq *pq, const float *vectors, int64_t n, int32_t iters, uint64_t seed,
                    void *stream);
/* The same for the sub-quantizers [sub_begin, sub_begin + sub_count) only.  The reference trains
 * the sub-quantizers as independent goroutines (pq.go:83-138); on several GPUs each rank trains a
 * range, the ranges are exchanged (vg_pq_get_codebooks_range -> all-gather -> vg_pq_set_codebooks)
 * and, the random stream being keyed by (seed, sub-quantizer), the result equals vg_pq_train's bit
 * for bit.  The quantizer counts as trained only after the full range [0, m) was trained in one
 * call or the codebooks were set. */
int32_t vg_pq_train_subset(vg_pq *pq, const float *vectors, int64_t n, int32_t iters, uint64_t seed,
                           int32_t sub_begin, int32_t sub_count, void *stream);
/* codebooks[sub_count*k*subdim], scales[sub_count], offsets[sub_count] of that range (trained or not) */
int32_t vg_pq_get_codebooks_range(vg_pq *pq, int32_t sub_begin, int32_t sub_count, int8_t *codebooks,
                                  float *scales, float *offsets);
/* Encode pq.go:147-176, batched: codes[n*m]; code = FindNearestCentroidInt8
 * (internal/simd/kernels.go:376-396: strict '<', lowest index wins ties) */
int32_t vg_pq_encode(vg_pq *pq, const float *vectors, int64_t n, uint8_t *codes, void *stream);
/* Decode pq.go:185-229, batched: out[n*dim] = float32(code)*scale + offset */
int32_t vg_pq_decode(vg_pq *pq, const uint8_t *codes, int64_t n, float *out, void *stream);
/* ComputeAsymmetricDistance pq.go:234-260 (no LUT, terms summed sequentially over the
 * sub-quantizers), one query against n codes: out[n] */
int32_t vg_pq_asymmetric_distance_batch(vg_pq *pq, const float *query, const uint8_t *codes,
                                        int64_t n, float *out, void *stream);

/* ---- OptimizedProductQuantizer (internal/quantization/opq.go, svd.go) ------------------------------------
 * A block-diagonal rotation in front of a ProductQuantizer; blocks = vg_opq_block_size (opq.go:38-58: the
 * multiple of dim/m dividing dim nearest 32; the whole vector up to 64 dims; blocks above 64 dims are refused).
 *   vg_opq_rotate     rotateVector (:196-215): out[b*bs+i] = simd.Dot(R_b[i], v_b), dotProductAvx512 order
 *   vg_opq_encode     Encode (:218-231) = rotate + ProductQuantizer.Encode        -> codes[n*m]
 *   vg_opq_decode     Decode (:234-269) = ProductQuantizer.Decode + R^T, summed left to right
 *   vg_opq_asymmetric_distance_batch   ComputeAsymmetricDistance (:272-286): rotate the query once, then PQ's
 *   vg_opq_train      Train (:89-193): num_iterations x { rotate all, ProductQuantizer.Train(pq_iters; the
 *                     reference's 20) from scratch with the stream seed + iteration, M_b = sum_i x_b^T yhat_b in
 *                     vector order, R_b = Procrustes(M_b) by one-sided Jacobi SVD (svd.go) }.  As in the reference
 *                     the last rotations are solved after the last PQ training.  Same seeded stream as
 *                     vg_pq_train: equals the CPU restatement bit for bit; the reference itself is unseeded.
 *   vg_opq_pq         the inner ProductQuantizer (codebooks: vg_pq_get_codebooks / vg_pq_set_codebooks)
 *   vg_opq_get/set_rotations   [nblocks][block][block] fp32 row-major, host memory. */
typedef struct vg_opq vg_opq;
int32_t vg_opq_block_size(int32_t dim, int32_t m);
int32_t vg_opq_create(vg_ctx *ctx, int32_t dim, int32_t m, int32_t k, int32_t num_iterations, vg_opq **out);
int32_t vg_opq_destroy(vg_opq *opq);
vg_pq *vg_opq_pq(vg_opq *opq);
int32_t vg_opq_is_trained(vg_opq *opq);
int32_t vg_opq_get_rotations(vg_opq *opq, int32_t *block, int32_t *nblocks, float *rotations);
int32_t vg_opq_set_rotations(vg_opq *opq, const float *rotations);
int32_t vg_opq_train(vg_opq *opq, const float *vectors, int64_t n, int32_t pq_iters, uint64_t seed, void *stream);
int32_t vg_opq_rotate(vg_opq *opq, const float *vectors, int64_t n, float *out, void *stream);
int32_t vg_opq_encode(vg_opq *opq, const float *vectors, int64_t n, uint8_t *codes, void *stream);
int32_t vg_opq_decode(vg_opq *opq, const uint8_t *codes, int64_t n, float *out, void *stream);
int32_t vg_opq_asymmetric_distance_batch(vg_opq *opq, const float *query, const uint8_t *codes, int64_t n,
                                         float *out, void *stream);

/* ---- RaBitQ / binary (internal/quantization/rabitq.go, binary.go) -------------------- */
/* BytesTotal rabitq.go:187-190: ((dim+63)/64)*8 + 4 */
int64_t vg_rabitq_code_bytes(int32_t dim);
/* Encode rabitq.go:51-78, batched: codes[n*code_bytes] = sign bits (bit i -> byte i/8, bit
 * i%8; v >= 0 sets the bit) padded to 8-byte words, then the little-endian fp32 norm
 * sqrt(Dot(v,v)) (dotProductAvx512 order, float64 sqrt rounded to fp32: simd/doc.go:58-60) */
int32_t vg_rabitq_encode(vg_ctx *ctx, int32_t dim, const float *vectors, int64_t n, uint8_t *codes,
                         void *stream);
/* Distance rabitq.go:119-176 of one query against n codes (reference layout): out[n] =
 * (|q|-|y|)^2 + (4*|q|*|y|/dim)*hamming, evaluated left to right in fp32 */
int32_t vg_rabitq_distance_batch(vg_ctx *ctx, int32_t dim, const float *query, const uint8_t *codes,
                                 int64_t n, float *out, void *stream);
/* simd.Hamming kernels.go:71 (hammingAvx512, popcount_avx512.c:25-46), one nbytes-long code
 * against n contiguous codes: out[n] (exact integers) */
int32_t vg_hamming_batch(vg_ctx *ctx, const uint8_t *a, const uint8_t *codes, int64_t nbytes, int64_t n,
                         int32_t *out, void *stream);

/* Test hooks (process-wide): force an alternative path so that tests can compare the paths bit for bit.
 * Names: VG_FLAT_NO_SMALL_TILE, VG_FLAT_UNFUSED, VG_FLAT_NO_SCAN, VG_FLAT_FORCE_EXACT, VG_FLAT_NO_DMA,
 * VG_FLAT_DEBUG, VG_PROBE_NO_GROUP, VG_ADC_BIGK_EXHAUSTIVE, VG_BUILD_DEBUG, VG_FLAT_RESCORE_SAMPLE, VG_PTHR_FORCE_HIST (the full list: Hook in
 * csrc/vg_internal.hpp).  The environment variable of the same
 * name ("1") gives the initial value, read once; the search entry points never call getenv. */
int32_t vg_debug_set_hook(const char *name, int32_t on);
/* Test entry point: a script of searcher.PriorityQueue operations (queue.go) replayed by ONE wave on the device
 * heap the graph searches use (csrc/vg_heap.hpp) — how the reference's own queue tests run against it.
 * ops[n_ops*4] = {op, node, float32 bits of distance, arg (capacity / maxSize)}; out[n_ops*3] = {flag, node, bits}:
 * flag = 1 pushed / accepted / item returned, 0 rejected / empty (VG_HEAP_LEN: the length).  is_max: NewPriorityQueue's
 * isMaxHeap; unsigned_keys != 0 selects the scalar-ALU sift-downs the walks use for distances >= +0.  final_items =
 * the heap array afterwards, item i = node | bits << 32; the script may hold at most cap (<= 8192) items. */
enum { VG_HEAP_PUSH = 0, VG_HEAP_POP = 1, VG_HEAP_PUSH_BOUNDED = 2, VG_HEAP_TRY_PUSH_BOUNDED = 3, VG_HEAP_TOP = 4,
       VG_HEAP_MIN_ITEM = 5, VG_HEAP_RESET = 6, VG_HEAP_LEN = 7 };
int32_t vg_debug_heap_replay(vg_ctx *ctx, int32_t is_max, int32_t unsigned_keys, const int32_t *ops, int32_t n_ops,
                             int32_t *out, int32_t *final_len, uint64_t *final_items, int32_t cap, void *stream);

/* ---- resident index ---------------------------------------------------------- */
int32_t vg_index_create(vg_ctx *ctx, int64_t n, int32_t dim, int32_t metric, vg_index **out);
int32_t vg_index_destroy(vg_index *idx);
/* PQ codes of a flat / DiskANN segment: n*m bytes row-major
 * (flat/segment.go:678-680 `codes[i*m:(i+1)*m]`, diskann/segment.go:316).  The
 * library keeps its own HBM copy (re-tiled for coalesced 16-byte loads); the
 * quantizer handle must outlive the index. */
int32_t vg_index_set_pq_codes(vg_index *idx, vg_pq *pq, const uint8_t *codes, void *stream);

/* RaBitQ codes of a DiskANN segment: n*code_bytes row-major (diskann/segment.go:1393-1409).
 * Re-tiled in HBM like the PQ codes (bits in 16-byte groups per 64-row tile, norms apart). */
int32_t vg_index_set_rabitq_codes(vg_index *idx, const uint8_t *codes, void *stream);

/* HNSW graph of a memtable shard (internal/hnsw): only the adjacency the search reads.
 *   l0[n*m0]            layer-0 neighbour ids in the node's stored order (node.go:62-80
 *                       GetConnectionsRaw order), VG_INVALID_ID terminates a shorter list;
 *                       m0 = 2*M <= 64 (hnsw.go:34-37 default M=32)
 *   max_level           highest level that has nodes (0 = layer 0 only)
 *   upper_slot[max_level*n]   for level L>=1: row of node in that level's table or VG_INVALID_ID
 *   upper_adj, level_rows[max_level]  tables of level_rows[L-1]*m ids each, concatenated
 *   entry_point         g.entryPointAtomic (hnsw.go:1800)
 * Needs vg_index_set_vectors (the scoring reads the fp32 rows). */
int32_t vg_index_set_hnsw_graph(vg_index *idx, int32_t m0, const uint32_t *l0, int32_t max_level,
                                int32_t m, const uint32_t *upper_slot, const uint32_t *upper_adj,
                                const int64_t *level_rows, uint32_t entry_point, void *stream);
/* HNSW construction over the index's fp32 rows: hnsw.Insert for rows 0..n-1 (hnsw.go:713-984 insert /
 * insertNode, :986-1106 selectNeighborsHeuristic, :455-555 addConnection / addConnectionPrune, :885-900
 * updateEntryPoint) with ApplyInsert's ids and levels (:629-684: id = row number, level =
 * layerForApplyInsert(id) :2103-2116, M0 = 2M :28).  Rows are inserted in id order in batches of
 * clamp(inserted / growth_div, 1, max_batch): every node of a batch searches the graph as it stood when
 * the batch began (what ApplyBatchInsert's goroutines see of one another), then the batch's links are
 * applied in id order; max_batch = 1 is the sequential Insert loop.  ef_construction = Options.EF
 * (hnsw.go:37 default 300).  The graph replaces the index's HNSW graph (vg_search_hnsw reads it).
 * 2 <= m <= 32, ef_construction <= 1024. */
int32_t vg_hnsw_build(vg_index *idx, int32_t m, int32_t ef_construction, int32_t max_batch,
                      int32_t growth_div, void *stream);
/* hnsw.ApplyInsert for `count` new rows (hnsw.go:629-637, insertNode :902-984), appended to the index as rows
 * n .. n+count-1 and linked into its HNSW graph: the memtable's write path.  rows: count*dim fp32, host or device.
 *   Ids and levels: new row t gets id t and level layerForApplyInsert(t), as in vg_hnsw_build (random levels of
 *     Insert's RNG are out of scope).  Existing nodes keep the levels the graph's slot table gives them (the graph
 *     may have been uploaded by vg_index_set_hnsw_graph from a CPU Insert).
 *   Batches: rows go in id order in batches of clamp(inserted / growth_div, 1, max_batch), `inserted` counting
 *     every node already in the graph; a call always ends a batch.  Hence vg_hnsw_build over b rows equals
 *     vg_hnsw_build over the first a rows followed by vg_hnsw_insert of rows a..b-1 whenever every call boundary is
 *     a batch boundary of the one-call schedule — for any a when max_batch = 1 (the sequential loop).
 *   Entry point: updateEntryPoint (hnsw.go:885-900) applies across calls: a new node above the top level becomes
 *     the entry point and its new levels are created.
 *   Empty index (n = 0, no graph): the first call creates the rows and the graph; repeated calls grow them.
 *   Everything sized by n follows: the fp32 rows, their norms, the bf16 filter image if enabled, the tombstone
 *     bitmap (new rows are live; tombstoned nodes stay in the graph and take part in the insert search, as
 *     insertNode searches unfiltered), and every search sees n + count rows afterwards.  The layer-0 edge
 *     distances of vg_index_set_hnsw_edge_distances are read by the insert and then dropped (the predicate-aware
 *     walk recomputes them, same values).
 *   Layout: the row arrays and the layer-0 table grow by capacity (x1.5); the upper levels are re-laid on every
 *     call (O(upper rows * m) ids), new nodes' rows appended to each level's table — the layout of a full build.
 *   Refusals, in this order: rows but no graph VG_ERR_NOT_READY; Hamming, m outside 2..32, ef_construction > 1024,
 *     >= 2^31 rows after the insert VG_ERR_UNSUPPORTED (max_batch / growth_div < 1 VG_ERR_INVALID_ARG); m not the
 *     graph's M or the graph's M0 not 2M VG_ERR_INVALID_ARG; PQ / SQ8 / INT4 / RaBitQ codes, IVF partitions, a
 *     Vamana graph or a nomination image (segment state) VG_ERR_UNSUPPORTED.  count = 0 changes nothing.
 *   Build state: a back link into an existing row needs the row's cached distances and the pair bits of its members.
 *     They are derived on the GPU, per call, for the rows the call's back links reach (cost scales with those rows,
 *     not n).  The pair bits are recomputed by the reference's pair kernel.  The cached distances cannot be: the
 *     insert search caches the bounded kernel's sum once its result heap is full, another summation order.  So the
 *     index keeps them for a graph it built or grew (4 B per slot, freed with the graph), and the equivalence above
 *     holds for such graphs.  For a graph from vg_index_set_hnsw_graph the layer-0 edge distances of
 *     vg_index_set_hnsw_edge_distances are used where given, else the pair kernel's distances: the same graph as the
 *     reference wherever those equal what the reference cached. */
int32_t vg_hnsw_insert(vg_index *idx, const float *rows, int64_t count, int32_t m, int32_t ef_construction,
                       int32_t max_batch, int32_t growth_div, void *stream);
/* layerForApplyInsert (hnsw.go:2103-2116) with layerMultiplier = 1/ln(m) (hnsw.go:218) */
int32_t vg_hnsw_level_for_id(uint64_t id, int32_t m);
/* HNSW.Compact (internal/hnsw/compact.go:16-34) on the index's graph under the tombstones of
 * vg_index_set_hnsw_tombstones: the memtable's answer to deletes.  Three phases, as written:
 *   1. repairActiveNodes / reconcileNode (:36-81, :174-233), every live node in id order.  checkRepairNeeded (:332-367):
 *      level l needs repair when its list has fewer than M/2 (integer division; l = 0: fewer than M) non-tombstoned
 *      members; a node with no such level is untouched.  greedyDescent (:235-258) from the entry point to the levels
 *      above the node's level gives (currID, currDist), the entry of EVERY level below (the reference never updates it,
 *      :226-231).  Per level: searchLayerPredicateAware (hnsw.go:1406-1557) on that level's lists with EF =
 *      ef_construction, the filter "id != node" and the tombstones as isDeleted; mergeCandidatesWithActiveNeighbors
 *      (:260-287): the results united with the node's non-tombstoned neighbours, an id present twice keeps the smaller
 *      distance (`<`), everything pushed back with PushItemBounded(EF); updateConnectionsForRepair (:289-328): the
 *      node's tombstoned neighbours are kept in slot order with their cached distances, selectNeighbors (heuristic,
 *      hnsw.go:1011-1106) takes max(limit - kept, 0) of the merged heap (limit M0 on layer 0, M above), the list becomes
 *      kept + selected, and only if something was selected (:315).
 *   2. pruneNodeConnections (:370-401): every live node's list on every level loses its tombstoned ids; the survivors
 *      keep their order and cached distances, freed slots are VG_INVALID_ID at the end.
 *   3. clearNodeConnections (:404-421): every tombstoned node's lists become empty — the entry point's too.  (The
 *      reference's test speaks of an exception for the entry point; its code makes none, and the code is what this
 *      reproduces.  A tombstoned entry point walks to nothing afterwards; the host re-elects one as recoverEntryPoint
 *      would, which is not part of this call.)
 *   Rules the reference leaves open: the merged set is pushed back in ascending id order (the reference ranges over a
 *     map).  A node's level is what the slot table gives it.  Levels that need no repair are walked by the reference
 *     without effect and skipped here (k_hnsw_compact.hip says why that changes nothing).
 *   Neighbor.Dist of a slot: vg_hnsw_insert's rule — the cached distance the index keeps for a graph it built or grew;
 *     for a graph from vg_index_set_hnsw_graph the layer-0 edge distances of vg_index_set_hnsw_edge_distances where
 *     given, otherwise the pair kernel's distance.  Distances the compaction computes are ComputeDistance
 *     (vectorstore/columnar.go:29-49): the pair kernel in the index's HNSW metric, `ok` always true.
 *   Batches: the nodes to repair are fixed up front (a repair writes only the node's own lists) and go in id order in
 *     batches of max_batch; every node of a batch walks the graph as it stood when the batch began, then the batch's
 *     lists are written.  max_batch = 1 is the reference with one worker; larger batches are what its GOMAXPROCS
 *     workers see of one another (the max_batch contract of vg_hnsw_build).
 *   Left as they are: the tombstones (still set), ids, rows, levels, the entry point and n.  The cached distances follow
 *     the lists: a built graph's are rewritten in place and its recomputed layer-0 edge distances, if any, dropped (as
 *     vg_hnsw_insert drops them); an uploaded graph's layer-0 edge distances are rewritten in place (computed first if
 *     the index had none), so that the predicate-aware walk and a later vg_hnsw_insert read what setConnections stored.
 *   The navigation queue, unbounded in the reference, has one slot per row: it cannot overflow, nothing is truncated.
 *   ef_construction = 0 means 300 (Options.EF).  stats may be NULL.  With no tombstones set, or none of them true, the
 *     call returns VG_OK, changes nothing and reports zeroed stats.
 *   Refusals, in this order, nothing changed: NULL index VG_ERR_INVALID_ARG; no HNSW graph or no fp32 rows
 *     VG_ERR_NOT_READY; max_batch < 1 VG_ERR_INVALID_ARG; Hamming, ef_construction > 1024, M outside 2..32 or
 *     M0 != 2M VG_ERR_UNSUPPORTED; PQ / SQ8 / INT4 / RaBitQ codes, IVF partitions, a Vamana graph or a nomination image
 *     (segment state, vg_hnsw_insert's list) VG_ERR_UNSUPPORTED.  (Present when the symbol is: see VG_ABI_MINOR.) */
typedef struct vg_hnsw_compact_stats { /* caller-allocated, may be NULL */
    int64_t repaired_nodes; /* live nodes with at least one list below its threshold */
    int64_t repaired_lists; /* (node, level) lists rewritten by the repair phase */
    int64_t pruned_links;   /* tombstoned ids removed from live nodes' lists (phase 2) */
    int64_t cleared_nodes;  /* tombstoned nodes whose lists were emptied (phase 3): those that still held a link */
} vg_hnsw_compact_stats;
int32_t vg_hnsw_compact(vg_index *idx, int32_t ef_construction, int32_t max_batch, vg_hnsw_compact_stats *stats,
                        void *stream);
/* The index's HNSW graph in vg_index_set_hnsw_graph's layout.  Every output may be NULL; call once for
 * the sizes (m0, m, max_level, level_rows[max_level]), then with buffers: l0[n*m0],
 * upper_slot[max_level*n], upper_adj[sum(level_rows)*m] (host or device). */
int32_t vg_index_get_hnsw_graph(const vg_index *idx, int32_t *m0, int32_t *m, int32_t *max_level,
                                uint32_t *entry_point, int64_t *level_rows, uint32_t *l0,
                                uint32_t *upper_slot, uint32_t *upper_adj, void *stream);
/* Vamana graph of a DiskANN segment: graph[n*r] (diskann/segment.go:671-681; VG_INVALID_ID =
 * empty slot), entry point = header.Entrypoint.  Scoring uses whichever of the index's data the
 * search call names. */
int32_t vg_index_set_vamana_graph(vg_index *idx, int32_t r, const uint32_t *graph, uint32_t entry_point,
                                  void *stream);
/* Vamana construction over the index's fp32 rows: diskann.Writer.buildGraph (diskann/writer.go:362-460) with
 * greedySearch (:472-569), robustPrune (:571-625) and addBackEdge (:627-643).  The graph and entry point replace the
 * index's Vamana graph as vg_index_set_vamana_graph would; vg_search_vamana (any kind) walks it.  (VG_ABI_MINOR 12.)
 * r, l, alpha of 0 take NewWriter's defaults (writer.go:84-110): 64, 100, 1.2.  1 <= r <= 64, 1 <= l <= 1024,
 * max_batch <= 16384 and n < 2^31, else VG_ERR_UNSUPPORTED; n == 0 is VG_ERR_INVALID_ARG ("no vectors to write");
 * no fp32 rows (vg_index_set_vectors) is VG_ERR_NOT_READY.
 * Distance: distance.Provider(metric) (distance/distance.go:97-106) in the pair kernel's summation order
 *   (squaredL2Avx512 / dotAvx512): SquaredL2 for L2; raw Dot for Cosine and Dot, sorted ASCENDING as the writer
 *   sorts it — the reference's quirk, reproduced: such a graph links the least similar rows.
 * Order: every sort ascends by (distance, id), distances compared as floats (-0 equals +0, every NaN after +Inf).
 *   The reference sorts by distance only over map iteration order; ties by id is the rule it leaves open.
 * Centroid and entry point (:386-404): centroid[j] = float32 sum over the rows in row order, divided by float32(n);
 *   the entry point is the first row with dist(row, centroid) < minDist, minDist starting at MaxFloat32 (row 0 when
 *   no row qualifies), fixed for the whole build.
 * Initial graph (:414-428): init_graph, if not NULL, is n*r ids (host or device), VG_INVALID_ID = empty slot (the
 *   row's ids keep their order, empty slots drop out); an id >= n, a self edge or an id twice in a row is
 *   VG_ERR_INVALID_ARG.  NULL: node i takes j = rng_u64(seed, i, P, t) % n for t = 0, 1, ... (the shared counter
 *   RNG, oracle vgo_rng_u64; P = 0x56414D414E41, "VAMANA"), skipping j == i and ids already taken, until it holds
 *   min(r, n-1) ids, in draw order.
 * Passes (:430-457): two passes over the nodes 0..n-1, the first with alpha 1, the second with alpha.  Per node i:
 *   1. results = greedySearch(row i, entry, l) as written: the pool is sorted every round; take the first
 *      unexpanded entry, stop if there is none or its index is >= l while the pool is longer than l; mark it
 *      expanded, cut the pool to l+50 if longer; append its unvisited neighbours (the entry starts visited);
 *      return the first l ids of the finally sorted pool.
 *   2. list(i) = robustPrune(i, results U list(i), r, alpha): the candidates without i sorted by d(c, i); c is kept
 *      while fewer than r are kept unless alpha * d(c, s) < d(c, i) (fp32) for a kept s, so a NaN keeps it.
 *   3. for each neighbour in list order, addBackEdge(neighbour, i): nothing if i is listed, else append i, and if
 *      the list is then longer than r, list = robustPrune(neighbour, list, r, alpha).
 * Batches: nodes go in id order in batches of clamp(processed / growth_div, 1, max_batch) (processed counts the nodes
 *   of both passes; a batch ends with its pass).  In a batch every node searches the graph as it stood when the
 *   batch began and prunes its own list as it stood then; all new lists are written; then the back edges are
 *   applied, each target's records in (source id, slot) order.  max_batch = 1 is the writer's sequential loop.
 * Output: lists in the order the reference leaves them (prune output sorted, back edges appended), padded with
 *   VG_INVALID_ID to r.  The writer's reorderBFS (reorder.go) is vg_vamana_reorder_bfs.  Deterministic: the same
 *   inputs give the same graph bit for bit. */
int32_t vg_vamana_build(vg_index *idx, int32_t r, int32_t l, float alpha, const uint32_t *init_graph, uint64_t seed,
                        int32_t max_batch, int32_t growth_div, void *stream);
/* FreshVamana.Insert (internal/segment/diskann/fresh_vamana.go:178-222) for `count` new rows, appended to the index as rows
 * n .. n+count-1 and linked into its Vamana graph: the streaming index's write path.  rows: count*dim fp32, host or device.
 * A node id is the row number (allocateNodeLocked :444-469).  r, l, alpha of 0 take FreshDefault* (:20-24): 64, 100, 1.2.
 *   Empty index (n = 0, no graph): the first call creates the rows and the graph; row 0 becomes the entry point and has no
 *     links (:198-201).  Otherwise the index's graph may come from vg_vamana_build, vg_index_set_vamana_graph or earlier
 *     calls; r must be the graph's.  VG_INVALID_ID slots are skipped wherever they sit; every list this call writes is a
 *     dense prefix padded with VG_INVALID_ID.
 *   deleted: bit i of byte i/8 = node i is deleted (FreshVamana.Delete is that one bit, the caller's to keep), ceil(n/8)
 *     bytes for the n rows that exist before the call, host or device, NULL = none; new rows are live.
 *   Distance: distance.Provider(metric) in the pair kernel's summation order, exactly as vg_vamana_build states it (raw Dot
 *     for Cosine and Dot, sorted ascending: the reference's quirk, reproduced).  In a sorted list -0 equals +0.
 *   Per node t:
 *   1. results = searchCandidatesLocked(row t, entry, l) (:616-671).  Two lists ordered by distance: candidates (cap 2l,
 *      popped from the front) and results (cap l, non-deleted nodes only; deleted nodes are still walked through).  The
 *      walk stops when results holds l items and the popped distance is greater than its last one, or candidates is empty.
 *      A popped node's unvisited neighbours are taken in list order.  insertCandidate (:898-923) places an item after
 *      every entry whose distance is <= its own and drops it when that position is >= cap: the order is (distance,
 *      arrival), which the reference pins.
 *   2. list(t) = robustPruneLocked(t, results, r, alpha) (:748-792): candidates in (distance, position) order; t itself and
 *      deleted ids are skipped; c is kept unless d(c, s) < alpha * c.dist for a kept s (the product is fp32, its own
 *      rounding step; a false comparison keeps c); stops at r kept.  The reference's sort.Slice moves nothing on the
 *      already ordered results and is a stable insertion sort on <= 12 items: the rule here is "stable by position"
 *      everywhere, which beyond 12 unordered items (the reverse edge's r + 1 candidates) is the rule the reference leaves open.
 *   3. for each neighbour in list order, addReverseEdgeLocked(neighbour, t) (:698-745): nothing if t is listed; appended
 *      while the list is shorter than r; at r the list in slot order followed by t, with distances to the neighbour, sorted
 *      stably by distance, goes through robustPruneLocked(neighbour, ..., r, alpha), which drops deleted ids and may keep
 *      fewer than r.
 *   4. maybeUpdateEntryPoint (:795-801) with count = t + 1: t becomes the entry point when count < 100, or when
 *      count % 500 == 0 and u < 0.1.  The reference's rand.Float32() is replaced (a stated deviation, like vg_vamana_build's
 *      initial graph) by u = float32(rng_u64(seed, count, P, 0) >> 40) * 2^-24, in [0, 1): the shared counter RNG (oracle
 *      vgo_rng_u64), P = 0x4652455348 ("FRESH").
 *   Batches: nodes go in id order in batches of clamp(nodes in the graph / growth_div, 1, max_batch); a call always ends a
 *     batch.  Every node of a batch searches the graph, and starts from the entry point, as they stood when the batch
 *     began; then the new lists are written; then the reverse edges are applied, each target's in (source id, slot) order.
 *     max_batch = 1 is the reference's serialized Insert loop (growMu).  Hence one call of a+b rows equals a call of a rows
 *     followed by a call of b rows whenever the call boundary is a batch boundary: for any a when max_batch = 1.
 *   NaN distances: a NaN orders after +Inf, in arrival order among NaNs, and compares greater than any number in the stop
 *     test (a stated deviation: sort.Search over a slice that NaNs left unordered is not restated).  Such inputs complete
 *     and leave a structurally valid graph.
 *   Everything sized by n follows: the fp32 rows, their norms, the bf16 filter image if enabled and the graph table grow by
 *     capacity (x1.5), and every search (vg_search_vamana*, vg_search_vamana_fresh), vg_vamana_reorder_bfs,
 *     vg_index_get_vamana_graph and vg_segment_write_diskann see n + count rows afterwards.  The visited bitmaps (n bits
 *     per searching node) of a launch stay under 1/16 of device memory; larger batches take several launches.
 *   Refusals, in this order, nothing changed: NULL index, count < 0 VG_ERR_INVALID_ARG; rows but no Vamana graph
 *     VG_ERR_NOT_READY; Hamming, r outside 1..64, l outside 1..1024, max_batch > 16384, >= 2^31 rows after the insert
 *     VG_ERR_UNSUPPORTED; max_batch < 1 or growth_div < 1 VG_ERR_INVALID_ARG; r not the graph's VG_ERR_INVALID_ARG; PQ / SQ8 /
 *     INT4 / RaBitQ codes, IVF partitions, an HNSW graph or tombstones, or a nomination image VG_ERR_UNSUPPORTED.
 *     count = 0 changes nothing.  (Present when the symbol is: see VG_ABI_MINOR.) */
int32_t vg_vamana_insert(vg_index *idx, const float *rows, int64_t count, int32_t r, int32_t l, float alpha,
                         const uint8_t *deleted, uint64_t seed, int32_t max_batch, int32_t growth_div, void *stream);
/* FreshVamana.consolidate (internal/segment/diskann/fresh_vamana.go:803-867) on the index's Vamana graph: every live node
 * that lists a deleted node gets a new list from a fresh search and prune, so that afterwards no live node lists a deleted
 * one.  The streaming index's delete path; the reference starts it once more than a tenth of the nodes are deleted
 * (:25-26, :261-266): that trigger, like the bitmap, is the caller's.
 *   Parameters: r is the graph's own.  l, alpha of 0 take FreshDefaultL / FreshDefaultAlpha: 100, 1.2.  deleted: bit i of
 *     byte i/8 = node i is deleted, ceil(n/8) bytes, host or device, any byte alignment; NULL = nothing is deleted: VG_OK,
 *     stats all zero, nothing written.  stats may be NULL and is written only on VG_OK.
 *   Repair set: the live nodes with a deleted id in any non-empty slot of their list, wherever the slot sits (VG_INVALID_ID
 *     slots are skipped as everywhere else), in ascending id order (:821-847).  A repair rewrites only the node's own list,
 *     and the test for a node reads only that list: the set is fixed before the first repair, by one pass over the graph as
 *     it stands at the call; only the walks depend on the order of the repairs.
 *   Per node i of the set (:859-862), steps 1 and 2 of vg_vamana_insert, word for word the same rules:
 *   1. results = searchCandidatesLocked(row i, entry, l): the same two lists with caps 2l and l, the same stop test, the
 *      (distance, arrival) order with -0 equal to +0, a NaN after +Inf in arrival order and greater than any number in the
 *      stop test; deleted nodes are walked through and stay out of results.  The node searches for its own row, so it
 *      normally meets itself at distance 0.
 *   2. list(i) = robustPruneLocked(i, results, r, alpha): i itself and deleted ids are skipped, the fp32 alpha * c.dist
 *      product, stops at r kept.  The new list is a dense prefix padded with VG_INVALID_ID, and may be shorter than the old
 *      one, or empty.
 *   No reverse edges are added and the entry point is never moved, even when it is itself deleted (walks still start there
 *     and pass through it).  Hence repaired lists usually come out shorter and recall can drop: the reference's behaviour,
 *     restated, not improved on.
 *   Batches: the repair set is cut into batches of max_batch nodes in id order; every node of a batch walks the graph as it
 *     stood when the batch began, then the batch's lists are written.  max_batch = 1 is the reference's loop.  There is no
 *     growth schedule: the graph does not grow.
 *   Idempotent: a repaired list holds no deleted id, a list that was not repaired held none; a second call with the same
 *     bitmap repairs nothing and changes no bit of the graph.
 *   Unchanged: n, the rows, the entry point (deleted or not), every list of a deleted node, and every list of a live node
 *     that named no deleted id, bit for bit, holes included.  No id is released.  Codes, partitions, nomination images and
 *     HNSW state on the index are neither needed nor touched (nothing is appended: none of vg_vamana_insert's segment-state
 *     refusals).  The visited bitmaps of a launch stay under 1/16 of device memory, as the insert's do.
 *   Refusals, in this order, nothing changed: NULL index VG_ERR_INVALID_ARG; (n == 0: VG_OK, stats zero, :815-818); no fp32
 *     rows or no Vamana graph VG_ERR_NOT_READY; Hamming, the graph's r outside 1..64, l outside 1..1024, max_batch > 16384
 *     (l result keys of scratch per batch node: 128 MiB at l = 1024) VG_ERR_UNSUPPORTED; max_batch < 1 VG_ERR_INVALID_ARG.
 *     (Present when the symbol is: see VG_ABI_MINOR.) */
typedef struct vg_vamana_consolidate_stats { /* caller-allocated, may be NULL */
    int64_t repaired_nodes; /* live nodes with at least one deleted id in their list */
    int64_t dropped_links;  /* slots of those lists that named a deleted id (an id listed twice counts twice) */
    int64_t links_before;   /* non-empty slots of the repaired nodes' lists before the call */
    int64_t links_after;    /* ... and after */
} vg_vamana_consolidate_stats;
int32_t vg_vamana_consolidate(vg_index *idx, int32_t l, float alpha, const uint8_t *deleted, int32_t max_batch,
                              vg_vamana_consolidate_stats *stats, void *stream);
/* The index's Vamana graph in vg_index_set_vamana_graph's layout: r, entry point, graph[n*r] (host or device);
 * graph NULL = the sizes only.  (VG_ABI_MINOR 12.) */
int32_t vg_index_get_vamana_graph(const vg_index *idx, int32_t *r, uint32_t *entry_point, uint32_t *graph,
                                  void *stream);
/* diskann.Writer.reorderBFS (diskann/reorder.go:14-157) on the resident index: perm[new] = old and inv_perm[old] = new
 * (the writer's addOrderToFinalRow), either NULL to skip, host or device.  (Present when the symbol is: see VG_ABI_MINOR.)
 * Order, bit for bit the writer's: a BFS over the index's Vamana graph from its entry point, each node's list in slot
 *   order, VG_INVALID_ID slots skipped wherever they sit; then, for i = 0 .. n-1 in id order, a fresh BFS from every i
 *   still unvisited.  Self edges and ids listed twice are harmless: a visited node is never queued again.
 * Afterwards the index is the segment the writer flushes: graph row new = old row perm[new] with every id mapped
 *   through inv_perm (slot order and VG_INVALID_ID slots keep their places), entry point inv_perm[entry] (= 0), and
 *   every per-row array permuted the same way: fp32 rows and their norms, the bf16 filter image, the PQ codes (rows,
 *   tiles, nomination image and norms), the RaBitQ codes (rows, tiles, norms; the largest |norm| stays), the SQ8 tiles
 *   and nomination image with its norms, the INT4 rows.  Row-count-invariant state (largest norms, quantizers, flat
 *   search counters) does not change.  The caller permutes what the index never held: ids, metadata, payloads.
 * Refusals, in this order, with nothing changed and nothing written: NULL index VG_ERR_INVALID_ARG; no Vamana graph
 *   VG_ERR_NOT_READY; an HNSW graph, HNSW tombstones, HNSW edge distances or IVF partitions (memtable / flat segment
 *   state) VG_ERR_UNSUPPORTED.  n = 0 is VG_OK with nothing done.
 * Memory: one scratch buffer of the largest permuted array and O(n) for the BFS, released before the call returns. */
int32_t vg_vamana_reorder_bfs(vg_index *idx, uint32_t *perm, uint32_t *inv_perm, void *stream);

/* fp32 rows of the segment, n*dim row-major — the layout of
 * vectorstore.ColumnarStore (internal/vectorstore/columnar.go:21-24) and of
 * flat.Segment.vectors (flat/segment.go:692).  Copied to HBM. */
int32_t vg_index_set_vectors(vg_index *idx, const float *base, void *stream);
/* Engine.CompactWithContext's Iterate loop (internal/engine/compaction.go:173-218; the memtable flush has the same shape with
 * one source and its HNSW tombstones) over resident indexes: the sources are walked in order, each in row order
 * (flat/segment.go:1028-1073), the rows whose bit is set in that source's tombstone bitmap are skipped (:179), the survivors
 * are appended to one new index, and the maps say where every row went (the loop's `moves`, :159-213).  Nothing crosses
 * PCIe but the bitmaps and the maps.  (Present when the symbol is: see VG_ABI_MINOR.)
 *   Sources: sources[0 .. n_sources-1], on `ctx`, of one dim and metric, each with its fp32 rows (vg_index_set_vectors, or
 *     an opened segment's).  Whatever else a source holds (codes, partitions, graphs, tombstones, nomination images) is
 *     neither needed nor touched: sources are read-only.  The same index may be listed twice; its rows then appear twice.
 *   deleted: NULL, or one pointer per source, any of them NULL: nothing is deleted there.  Otherwise vg_vamana_consolidate's
 *     convention: bit i of byte i/8 = row i is deleted, ceil(n_s/8) bytes, host or device, any byte alignment; bits at or
 *     above n_s are ignored.
 *   *out: a new index on `ctx` with the sources' dim and metric, to be destroyed with vg_index_destroy.  Its rows are the
 *     live rows of source 0 in ascending row order, then those of source 1, and so on, bit for bit; its norms are what
 *     vg_index_set_vectors computes for those rows, bit for bit, and the largest norm and largest |x| are taken over the
 *     merged rows (a deleted row may have held a source's maximum); capacities are exact and the flat search counters zero,
 *     as after vg_index_set_vectors.  No codes, graph, partitions or bf16 image are carried over: the writer that follows
 *     (vg_flat_build, vg_diskann_build) retrains and rebuilds, as the reference's does.
 *   Maps, each NULL to skip, host or device: old_to_new[off_s + i] = the new row of source s row i, or VG_INVALID_ID if that
 *     row is deleted, off_s = the row counts of the sources in front (sum of all n_s entries); new_source[j], new_row[j] =
 *     where new row j came from (one entry per live row; a caller that has not counted them sizes both for the sum).
 *   No live row: VG_OK, *out has 0 rows (as vg_index_create with n = 0), old_to_new is all VG_INVALID_ID.
 *   Refusals, in this order, *out NULL and nothing written: NULL ctx, sources or out, n_sources < 1, a NULL source
 *     VG_ERR_INVALID_ARG; a source on another context VG_ERR_INVALID_ARG; a source of another dim VG_ERR_DIM_MISMATCH; a
 *     source of another metric VG_ERR_INVALID_ARG; metric Hamming VG_ERR_UNSUPPORTED; a source with rows but no fp32 rows
 *     VG_ERR_NOT_READY; the sources' row counts (deleted rows included: the test comes before any allocation) summing to
 *     0xFFFFFFFF or more VG_ERR_INVALID_ARG.  A failure after these (out of memory, a HIP error) returns its status with
 *     *out NULL, nothing kept and the maps unspecified.
 *   The result's row count is the number of old_to_new entries other than VG_INVALID_ID, or the sources' row counts less the
 *     set bits below n_s of their bitmaps: there is no getter for an index's row count, so a caller that passes no
 *     old_to_new counts its bitmaps.
 *   Work: four kernel launches whatever the rows and however many sources.  Memory: the new rows (sources and result
 *     coexist), plus scratch released before the call returns: two 4-byte words per live row (the (source, row) lists,
 *     whether or not the caller asks for them), one per 2048 source rows, 48 bytes per source (the descriptors); and what
 *     is staged for the host: 4 bytes per source row for an old_to_new in host memory (a device one is written where it
 *     lies), n_s/8 bytes per bitmap in host memory (device ones are read where they lie).  Waits for `stream` (the row
 *     count is read back). */
int32_t vg_index_merge(vg_ctx *ctx, const vg_index *const *sources, const uint8_t *const *deleted, int32_t n_sources,
                       vg_index **out, uint32_t *old_to_new, int32_t *new_source, uint32_t *new_row, void *stream);

/* ---- Metadata filters on the device: resident columns -> row masks ------------------
 * Every filtered search of this header takes its filter as one bit per row (mask / mask_stride).  These calls make those
 * bits on the device from the segment's metadata columns, so a filtered batch needs only its predicates from the host: the
 * counterpart of simd.FilterRangeF64 / FilterRangeF64Indices / CountRangeF64 / GatherU32 (internal/simd/kernels.go:126-170)
 * and of AndWords / AndNotWords / OrWords / XorWords / PopcountWords (bitmap.go:26-55).  (Present when the symbols are:
 * see VG_ABI_MINOR.)
 *
 * Semantics: the reference's.  A filter set is the AND of its filters (internal/metadata/unified.go:279-416,
 *   metadata.FilterSet); an empty filter set matches every row (:280-282); a filter on a field the segment has no column
 *   for matches nothing (numeric_index.go:1065-1068, unified.go:318-321).
 *   Numeric fields (f64 columns; ops eq ne lt lte gt gte): a row matches iff it has a value for the field and
 *   compareFloat64(value, op, filterVal) holds (numeric_index.go:1020-1037, the definition MatchRowID uses); int values
 *   are stored as float64(I64) (:1072-1076).  Rows without the field never match, `ne` included (the reference's `ne`
 *   starts from the rows that have the field, :1176-1182, :1211-1228).  The reference's range path with math.Nextafter
 *   (:488-497) equals the strict compare for every non-NaN value.  For a stored NaN under `ne` the reference's own paths
 *   disagree: the bitmap path and compareFloat64 keep the row, the sorted column scan drops it.  THIS LIBRARY FOLLOWS
 *   compareFloat64 (a stated choice): the compares are IEEE compares, -0 equals +0, a NaN filter value matches nothing
 *   except under `ne`, where it matches every present row, and a stored NaN matches only `ne`.
 *   Categorical fields (code columns; ops eq and in): the reference keeps one bitmap per (key, value) (unified.go:316-348,
 *   getBitmapLocked :1614); the device form is one uint32 dictionary code per row, VG_INVALID_ID = the row has no value;
 *   the value -> code dictionary is the host's.  `eq` matches the rows whose code is the clause's, `in` the rows whose
 *   code is in the clause's set (duplicates allowed); an empty set matches nothing (:327-330); a row without a value
 *   matches nothing, also when the clause names VG_INVALID_ID itself.  Any other op on a code column, and `in` on an f64
 *   column, is VG_ERR_UNSUPPORTED.
 *   deleted: NULL, or one bitmap for the batch (bit i of byte i/8 = row i is deleted, ceil(rows/8) bytes, any byte
 *   address): cleared from every query's mask in the same pass ("tombstones are the caller's: clear their bits").
 *   Out of scope, the host's: `contains`, string ranges, array-valued fields, block statistics; a mask made on the host
 *   joins a device one through vg_mask_combine.  Columns do not follow writes: the host uploads a column again.
 *
 * vg_columns: the resident columns of ONE segment of `rows` rows (rows < 2^31, else VG_ERR_UNSUPPORTED), fields 0..63 (the
 *   caller's handle for a key).  vg_columns_set_f64: values[rows]; present: bit i of byte i/8 = row i has a value, NULL =
 *   every row.  vg_columns_set_codes: codes[rows].  Both copy (host or device source), replace whatever the field held
 *   (f64 or codes) and wait for `stream`, as vg_index_set_* do; vg_columns_drop leaves the field without a column (it then
 *   matches nothing); create / set / drop / destroy are serialised by the caller against evaluations of the same columns.
 *   Memory: 8 (f64) or 4 (codes) bytes per row, rows rounded up to VG_FILTER_TILE_ROWS, plus one presence bit per row.
 *
 * vg_filter_evaluate: query q's filter set = clauses[clause_off[q] .. clause_off[q+1]); clause_off has nq + 1 entries.
 *   Bytes written: exactly ceil(rows/8) bytes per query at mask + q * mask_stride; mask_stride >= that many bytes
 *   (mask_stride == 0 only for nq <= 1); bits at positions >= rows in the last byte are zero; the bytes between
 *   ceil(rows/8) and mask_stride are left untouched.  counts[q] = the set bits of query q's mask (the selectivity
 *   numerator of vg_search_hnsw_filtered and of the flat searches' callers); may be NULL.
 *   Pointers: host or device, each on its own; mask may sit at any byte address with any stride — 8-byte word stores
 *   where mask and mask_stride are 8-byte aligned, byte stores otherwise, the same bits.  With every buffer on the device
 *   the call only enqueues on `stream`; a host buffer makes it wait.
 *   Limits: at most 16 clauses per query, at most 4096 codes per `in` set: beyond them VG_ERR_UNSUPPORTED with the number
 *   in the message.  VG_ERR_INVALID_ARG: a field outside 0..63, an unknown op, a non-monotone or negative clause_off, a set
 *   range outside [0, n_sets), NULL cols / clause_off / mask, mask_stride below ceil(rows/8).  These are tested on the
 *   arrays the host can read, before any work; clause arrays in DEVICE memory are the caller's to keep well formed (the
 *   call does not read them back: a query then takes at most its first 16 clauses, and a clause with a field outside
 *   0..63, an op its column does not have or a set range outside `sets` matches nothing).  A valid field with no column
 *   set is no error: it matches nothing.  nq == 0: VG_OK.  rows == 0: VG_OK, no mask byte is written, counts are 0.
 *   Work: one kernel launch; a workgroup owns VG_FILTER_TILE_ROWS rows, stages the column slices its queries name in LDS
 *   once and loops over its queries ("Filter evaluation").
 *
 * vg_mask_combine: dst[q] = dst[q] OP src[q] over the ceil(rows/8) bytes of each of nq masks (VG_MASK_ANDNOT: dst & ~src,
 *   simd/bitmap.go:26-48); src_stride 0 = one src for every query (a host-made mask, a tombstone bitmap); whole bytes:
 *   the last byte's bits at or above `rows` are combined like the others.  nq <= 65535.  dst and src must not overlap.
 * vg_mask_popcount: counts[q] = the set bits below `rows` of mask + q * mask_stride (bitmap.go:50-55); bits at or above
 *   `rows` that the caller left set in the last byte are not counted.  Both take host or device pointers at any byte
 *   address (8-byte words where everything is 8-byte aligned, bytes otherwise and at the tail) and only enqueue when
 *   every buffer is on the device.
 * vg_mask_alloc / vg_mask_free: `bytes` of zero-filled device memory for masks, for a host that has no HIP binding of its own
 *   (the cgo shim): what vg_filter_evaluate fills and the filtered searches read.  bytes == 0 gives NULL; freeing NULL is
 *   VG_OK; vg_mask_free waits for the device. */
#define VG_FILTER_TILE_ROWS 4096 /* rows of one workgroup of vg_filter_evaluate: the tests' row seams */
typedef struct vg_columns vg_columns;
int32_t vg_columns_create(vg_ctx *ctx, int64_t rows, vg_columns **out);
int32_t vg_columns_destroy(vg_columns *cols);
int32_t vg_columns_set_f64(vg_columns *cols, int32_t field, const double *values, const uint8_t *present, void *stream);
int32_t vg_columns_set_codes(vg_columns *cols, int32_t field, const uint32_t *codes, void *stream);
int32_t vg_columns_drop(vg_columns *cols, int32_t field);

enum { VG_FILTER_EQ = 0, VG_FILTER_NE, VG_FILTER_LT, VG_FILTER_LTE, VG_FILTER_GT, VG_FILTER_GTE, VG_FILTER_IN };
typedef struct vg_filter_clause { /* 32 bytes, caller-allocated */
    int32_t field, op;
    double value;                 /* f64 columns */
    uint32_t code;                /* code columns, VG_FILTER_EQ */
    int32_t set_begin, set_count; /* code columns, VG_FILTER_IN: sets[set_begin .. set_begin + set_count) */
    int32_t reserved;             /* 0 */
} vg_filter_clause;
int32_t vg_filter_evaluate(vg_columns *cols, const vg_filter_clause *clauses, const int32_t *clause_off, int64_t nq,
                           const uint32_t *sets, int64_t n_sets, const uint8_t *deleted, uint8_t *mask, int64_t mask_stride,
                           int64_t *counts, void *stream);

enum { VG_MASK_AND = 0, VG_MASK_ANDNOT, VG_MASK_OR, VG_MASK_XOR };
int32_t vg_mask_combine(vg_ctx *ctx, int32_t op, uint8_t *dst, int64_t dst_stride, const uint8_t *src, int64_t src_stride,
                        int64_t nq, int64_t rows, void *stream);
int32_t vg_mask_popcount(vg_ctx *ctx, const uint8_t *mask, int64_t mask_stride, int64_t nq, int64_t rows, int64_t *counts,
                         void *stream);
int32_t vg_mask_alloc(vg_ctx *ctx, int64_t bytes, uint8_t **out);
int32_t vg_mask_free(vg_ctx *ctx, uint8_t *mask);

/* ---- pre-filter search: score only the rows a filter keeps -------------------------------------
 * The engine's bitmap strategy (internal/engine/search.go:500-737): when a query's filter keeps few rows, Engine.SearchIter
 * does not scan.  It turns the filter result into row ids (ToArrayInto, :617-627), drops tombstones and sorts the ids
 * (:633-678), fetches exactly those rows and scores them with distance.SquaredL2 / distance.Dot (:699-713), and keeps the best
 * searchK in one CandidateHeap (:717-733).  The host chooses this path, as the engine does (selectivityCutoff /
 * adaptiveThreshold, :572-586), from the counts vg_filter_evaluate gave it; no other search of this header routes here.
 * (Present when the symbols are: see VG_ABI_MINOR.)
 *
 * vg_mask_to_rows: ToArrayInto for a batch of masks.  Per query q the ids of the set bits below `rows` of
 *   mask + q * mask_stride, ascending, go to out_rows + q * out_stride: at most out_stride of them; the slots from the number
 *   written up to out_stride are set to VG_INVALID_ID, so the block feeds vg_rerank / vg_score_candidates as it is.
 *   counts[q] = ALL set bits below `rows`, also when that exceeds out_stride (the caller sees a truncation); may be NULL.
 *   Bits at or above `rows` in the last byte are ignored, as vg_mask_popcount ignores them.  Masks: any byte address and any
 *   stride >= ceil(rows/8) (mask_stride == 0 only for nq <= 1); host or device pointers, each on its own; with every buffer
 *   on the device the call only enqueues.  nq == 0 or rows == 0: VG_OK (counts 0, every slot VG_INVALID_ID).  out_stride == 0
 *   with counts set is a count only.  rows < 2^31.  Work: a workgroup compacts VG_MASK_ROWS_TILE_ROWS rows of one mask (tile
 *   counts, a scan per mask, a scatter: row order is kept and a single mask still spreads over the chip).
 *
 * vg_search_flat_prefilter: search.go:602-736 over ONE resident segment.  Query q's candidates are the rows whose bit is set
 *   in its mask (mask_stride == 0: one mask for the batch; tombstones are the caller's: it clears their bits); each is scored
 *   from the fp32 rows with distance.SquaredL2 (L2) or distance.Dot (Dot, Cosine) in squaredL2Avx512 / dotProductAvx512 order;
 *   ids/scores[nq*k] = the best k by (Score, RowID), best first, padded with VG_INVALID_ID and +Inf (L2) / -Inf (Dot, Cosine).
 *   IVF partitions on the index are IGNORED — the strategy fetches rows by id and never probes: on an index with at most one
 *   partition the result equals vg_search_flat_filtered(..., VG_SCAN_F32, ...) bit for bit, on a partitioned one that of the
 *   same rows without partitions.  Codes, graphs and nomination images on the index are neither needed nor touched.
 *   NaN scores: the CandidateHeap replayed with the engine's `Pop(); Push(c)` at capacity (search.go:725-733; see "NaN scores").
 *   k <= 16384 (searchK = k * RefineFactor is the caller's).  The call WAITS for `stream` once: the masks' population counts
 *   size the row lists.  Query chunks keep lists and keys inside the context's scratch cap.  A listed row costs one
 *   16-lane exact product per query; the list of a query is cut into chunks of VG_PREFILTER_CHUNK_ROWS rows, one workgroup
 *   each; with one mask for the batch a workgroup stages its listed rows in LDS and scores them against a group of queries.
 *   Refused before any work: NULL index / buffers, negative nq or k, mask == NULL (a search without a filter is
 *   vg_search_flat), mask_stride below ceil(rows/8) with nq > 1: VG_ERR_INVALID_ARG; Hamming: VG_ERR_UNSUPPORTED; rows but no
 *   fp32 rows: VG_ERR_NOT_READY; k > 16384: VG_ERR_UNSUPPORTED with the number in the message.  nq == 0 or k == 0 writes
 *   nothing; an index of 0 rows gives padding only. */
#define VG_MASK_ROWS_TILE_ROWS 8192 /* rows of one workgroup of the compaction (vg_mask_to_rows): the tests' row seams */
#define VG_PREFILTER_CHUNK_ROWS 256 /* listed rows of one workgroup of vg_search_flat_prefilter's score kernels */
int32_t vg_mask_to_rows(vg_ctx *ctx, const uint8_t *mask, int64_t mask_stride, int64_t nq, int64_t rows, uint32_t *out_rows,
                        int64_t out_stride, int64_t *counts, void *stream);
int32_t vg_search_flat_prefilter(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask,
                                 int64_t mask_stride, uint32_t *ids, float *scores, void *stream);

/* ---- hybrid search: a resident BM25 index and Reciprocal Rank Fusion ---------------------------------
 * Engine.HybridSearch (internal/engine/engine.go:1538-1640) takes a vector top-max(2k, 50) and a BM25 top-max(2k, 50) from
 * lexical/bm25 (MemoryIndex.Search, bm25.go:282-381) and fuses them by Reciprocal Rank Fusion (:1560-1602).  The host keeps
 * what is text: the tokeniser, the string -> term id dictionary, math.Log (the idf) and the doc / row -> primary key maps; the
 * device gets the inverted index as CSR postings and answers batches.  (Present when the symbols are: see VG_ABI_MINOR.)
 *
 * vg_bm25: the resident index.  Term t's posting list is post_doc / post_tf[term_off[t] .. term_off[t + 1]) (docID, count:
 *   bm25.go:18-21); doc_len[d] = idx.docLengths[d] (0 for a deleted doc's slot); total_length = idx.totalLength and
 *   doc_count = idx.docCount (passed on their own because deleted docs keep a slot); doc_to_id[d] = the id doc d is reported
 *   and fused under (one resident segment: its row id), NULL = d itself.  vg_bm25_create copies (each array from host or
 *   device memory) and waits once; writes reach the index through vg_bm25_update (below), not through another upload.
 *   STATED DEVIATION: every posting list must be in STRICTLY ASCENDING doc order.  The reference's lists are in insertion
 *   order, and after deleteLocked's swap-remove (bm25.go:252-254) and the reuse of freed doc ids (:191-195) they can be out of
 *   order; its document-at-a-time walk then meets such a doc more than once and scores it in pieces — an artefact, not a
 *   contract.  The host sorts the lists before the upload (the cgo shim does).  Arrays in HOST memory are checked: a list out
 *   of order, or a doc id >= n_docs, is VG_ERR_INVALID_ARG naming the term.  Arrays in DEVICE memory are NOT validated (the
 *   call does not read them back): they are the caller's to keep well formed; term_off is read back and checked either way.
 *   Limits: n_docs < 2^31 and fewer than 2^63 postings (VG_ERR_UNSUPPORTED with the number), doc_count >= 1
 *   (VG_ERR_INVALID_ARG with the number: the reference answers nothing for an empty index, bm25.go:286).
 *   vg_bm25_stats: docs, terms, postings and the resident bytes (any pointer may be NULL).
 *
 * vg_bm25_search: query q's terms are q_terms[q_term_off[q] .. q_term_off[q + 1]) (term ids; an id >= n_terms is a term the
 *   dictionary does not have: an empty list, which contributes nothing, bm25.go:302) with one idf per entry in q_idf.  THE IDF
 *   COMES FROM THE CALLER: computeIDF (:383-387) is math.Log in float64, and Go's Log is not the device's; the host computes
 *   math.Log(1 + (N - n + 0.5) / (n + 0.5)) and the device multiplies by exactly those doubles.  A term named twice is two
 *   iterators and adds twice.  The answer is MemoryIndex.Search's, bit for bit: per doc, in float64 and nothing fused,
 *   num = tf * (k1 + 1), denom = tf + k1 * (1 - b) + (k1 * b / avgDL) * docLen, score += idf * (num / denom), the constants
 *   formed as bm25.go:314-317 forms them, the terms added IN THE QUERY'S TERM ORDER; a doc takes part when its float64 score
 *   is > 0; the heap compares float32(score).  out_ids[nq * k] (through doc_to_id) and out_scores[nq * k] best first,
 *   out_counts[q] = min(k, hits) (NULL: not wanted), the tail VG_INVALID_ID / -Inf.
 *   Ties: candidateHeap (:394-441) is a binary min-heap that compares scores only, so among equal scores its layout decides
 *   (k = 2 and scores 1, 1, 2 in doc order answer [C, B], not [C, A]).  The key selection answers a query exactly when its
 *   best k scores are pairwise different and no further doc shares the k-th score; every other query is replayed through the
 *   reference's push / up / down / pop over its docs in ascending order.  vg_bm25_replayed: the queries replayed since
 *   vg_bm25_create (waits for `stream`), as vg_index_flat_retried counts the flat search's.
 *   Work: a workgroup owns VG_BM25_TILE_DOCS docs of one query (their float64 sums in LDS) and walks each term's sub-range
 *   of that tile in term order; the docs with a score become keys; the best k of each list are selected as the threshold
 *   searches select theirs.  The lists are sized by the terms' list lengths: the query arrays are read on the host, so query
 *   arrays in device memory make the call wait for `stream` once; query chunks keep the lists inside the context's scratch cap.
 *   Pointers: host or device, each on its own, element-aligned.  Limits: k <= 16384 and at most 64 terms per query, beyond
 *   them VG_ERR_UNSUPPORTED with the number in the message.  nq == 0 or k == 0 writes nothing; a query without terms and
 *   k > hits are served.
 *
 * vg_rrf_fuse: engine.go:1560-1602 for a batch.  Query q's list A is a_ids[q * a_stride ..] of a_counts[q] entries (cut to
 *   a_stride), list B likewise; a NULL ids or counts pointer, or a count of 0, is an empty list; VG_INVALID_ID entries are
 *   skipped but keep their rank.  Rank r of list A SETS the id's score to 1.0f / float32(rrf_k + r + 1) — an id named twice
 *   in A keeps its last rank, as the map assignment does; every rank of list B then ADDS the same term in float32, in
 *   ascending rank.  out_ids / out_scores[nq * k]: the k best by score descending, the tail VG_INVALID_ID / -Inf;
 *   out_counts[q] = min(k, distinct ids) (NULL: not wanted).  TIES ARE DEFINED AS ASCENDING ID.  The reference sorts the
 *   entries of a Go map with an unstable sort, so its order inside equal scores — and which ids of a tied group it cuts at
 *   k — is undefined; the result here is always one of the answers the reference can give.  The division is correctly rounded.
 *   One workgroup per query sorts the two lists' (id, source, rank) keys in LDS, combines equal ids and sorts (score, id).
 *   Limit: a_count + b_count <= 16384 per query (128 KiB of keys; HybridSearch up to k = 4096) and k <= 16384, beyond them
 *   VG_ERR_UNSUPPORTED with the number; counts in device memory are not read back: their strides are taken as the counts.
 *   With every buffer on the device the call only enqueues. */
#define VG_BM25_TILE_DOCS 8192 /* docs of one workgroup of vg_bm25_search's score kernel: the tests' doc seams */
typedef struct vg_bm25 vg_bm25;
int32_t vg_bm25_create(vg_ctx *ctx, int64_t n_docs, int64_t n_terms, const int64_t *term_off, const uint32_t *post_doc,
                       const uint32_t *post_tf, const uint32_t *doc_len, int64_t total_length, int64_t doc_count,
                       const uint32_t *doc_to_id, vg_bm25 **out);
int32_t vg_bm25_destroy(vg_bm25 *bm);
int32_t vg_bm25_stats(vg_bm25 *bm, int64_t *docs, int64_t *terms, int64_t *postings, int64_t *bytes);
int32_t vg_bm25_search(vg_bm25 *bm, const int32_t *q_term_off, const uint32_t *q_terms, const double *q_idf, int64_t nq, int32_t k,
                       uint32_t *out_ids, float *out_scores, int32_t *out_counts, void *stream);
int32_t vg_bm25_replayed(vg_bm25 *bm, int64_t *replayed, void *stream);
/* Writes to the resident index, without a rebuild.  (Present when the symbols are: see VG_ABI_MINOR.)
 *
 * vg_bm25_update: one call is a batch of MemoryIndex.deleteLocked (bm25.go:238-278) followed by a batch of Add (:180-229),
 *   applied to the CSR image where it lies: the host no longer sorts and uploads the whole index after a write.
 *   Deletes: every posting of a doc in del_docs[n_del] leaves its list, doc_len[d] becomes 0 and doc_to_id[d] 0 (:268-269); a
 *   doc named twice, or one without postings, is fine.  Adds: added doc i is add_docs[i], of length add_len[i], reported under
 *   add_ids[i], with the postings (add_terms[p], add_tf[p]) for p in add_off[i] .. add_off[i + 1] — the document-major form
 *   in which a host's tf map arrives (:205-228); add_docs in any order; a doc in both lists is a replace (deletes apply
 *   first).  The host allocates doc ids: the free list of :191-195 stays with it, as the dictionary does.
 *   Afterwards the index is bit for bit the one vg_bm25_create would hold for the updated index, with STABLE TERM IDS: term
 *   t's list is its old list without the deleted docs together with its added postings, strictly ascending by doc; a list
 *   that empties stays as an empty range (the reference deletes it, :259-261: the host skips a term whose df is 0); the ids
 *   from the old n_terms up to n_terms_new are new terms, unused ones empty ranges.  n_docs grows to n_docs_new, slots
 *   without a document have length 0 (and id 0); neither size may shrink (VG_ERR_INVALID_ARG with the number).
 *   total_length and doc_count come from the caller as in vg_bm25_create and the three constants are formed as there;
 *   doc_count == 0 afterwards is allowed (the index then answers nothing).  vg_bm25_replayed keeps counting across updates.
 *   doc_to_id: an index made with the array (or vg_bm25_create_empty(.., 1, ..)) requires add_ids; an identity index refuses
 *   a non-NULL add_ids (VG_ERR_INVALID_ARG).
 *   FAILURE IS ATOMIC: the next image is built beside the current one; an error flag is read back together with the new
 *   offsets (whose host copy vg_bm25_search sizes its key lists from), and that readback is the call's one wait for `stream`
 *   — besides add_off in device memory, which is read back first (it sizes the call, as term_off does in vg_bm25_create), and
 *   an array that has to grow.  After a failed call the index is exactly as it was.
 *   Checks: arrays in HOST memory are validated before anything is enqueued — a doc >= n_docs_new, a deleted doc >= the old
 *   n_docs, a term >= n_terms_new, a doc named twice in add_docs, a term named twice inside one doc, a decreasing add_off:
 *   VG_ERR_INVALID_ARG naming the doc or the term.  Arrays in DEVICE memory are not validated, the rule vg_bm25_create
 *   states (ids out of range are caught on the device all the same: VG_ERR_INVALID_ARG, nothing is written out of range).  One
 *   check is made on the device for either kind: an added doc that still has a surviving posting in a list it is added to
 *   (an add into a live slot) is VG_ERR_INVALID_ARG naming the doc.
 *   Limits (VG_ERR_UNSUPPORTED with the number): n_docs_new < 2^31, term ids are uint32, fewer than 2^31 added postings per
 *   call.  n_del == 0, n_add == 0 or both are served.  More than 2^32 postings are NOT TESTED: posting offsets are int64
 *   throughout by construction, a test of that size does not run in seconds.
 *   Memory: the postings and the offsets ping-pong between two buffers with capacity (the second appears at the first
 *   update; a buffer too small for old + added postings is replaced by one of max(need, 1.5 x the larger of the two));
 *   doc_len / doc_to_id grow by the same rule and are written only after the error check has passed.  vg_bm25_stats reports
 *   the bytes actually held: 8 per offset slot and 8 per posting slot of BOTH images, 4 (8 with doc_to_id) per doc slot.
 *   A search on ANOTHER stream that overlaps an update is the caller's to order: it may read buffers the update rewrites.
 *   Work: one streaming pass over the old postings marks them live or deleted and ranks them (VG_BM25_UPDATE_CHUNK postings
 *   per workgroup), the added postings are radix-sorted by (term, doc), a scan over n_terms_new gives the new offsets, and a
 *   second streaming pass writes every posting to its final position: HBM bytes, proportional to the index, not a host sort
 *   plus a PCIe upload of it.
 * vg_bm25_create_empty: an index with no docs, no terms and doc_count 0 (vg_bm25_create keeps refusing one); with_doc_to_id
 *   != 0: it reports through a doc_to_id array that the updates' add_ids fill.  vg_bm25_search on an index whose doc_count is
 *   0 writes the empty answer (VG_INVALID_ID / -Inf, counts 0), as bm25.go:286 answers nothing.
 * vg_bm25_export: the image copied out, each array to host or device memory, any pointer NULL = not wanted; sizes from
 *   vg_bm25_stats (term_off: terms + 1).  What a host needs to persist an index it never built. */
#define VG_BM25_UPDATE_CHUNK 2048 /* postings one workgroup of the update's passes owns: the tests' posting seams */
int32_t vg_bm25_create_empty(vg_ctx *ctx, int32_t with_doc_to_id, vg_bm25 **out);
int32_t vg_bm25_update(vg_bm25 *bm, const uint32_t *del_docs, int64_t n_del, const uint32_t *add_docs, const uint32_t *add_len,
                       const uint32_t *add_ids, int64_t n_add, const int64_t *add_off, const uint32_t *add_terms, const uint32_t *add_tf,
                       int64_t n_docs_new, int64_t n_terms_new, int64_t total_length, int64_t doc_count, void *stream);
int32_t vg_bm25_export(vg_bm25 *bm, int64_t *term_off, uint32_t *post_doc, uint32_t *post_tf, uint32_t *doc_len, uint32_t *doc_to_id,
                       void *stream);
int32_t vg_rrf_fuse(vg_ctx *ctx, int64_t nq, const uint32_t *a_ids, const int32_t *a_counts, int64_t a_stride, const uint32_t *b_ids,
                    const int32_t *b_counts, int64_t b_stride, int32_t rrf_k, int32_t k, uint32_t *out_ids, float *out_scores,
                    int32_t *out_counts, void *stream);

/* ---- L0 batch kernels: the dispatch seam (internal/simd/kernels.go:11-30) ------- */
/* simd.SquaredL2Batch / simd.DotBatch (kernels.go:61-68 → batch_avx512.c:19-143):
 * one query against n contiguous targets; out[n].  Bit-identical to the AVX-512
 * kernels (4x16 FMA accumulators, 16-wide tail, reduce_add tree, FMA scalar tail). */
int32_t vg_squared_l2_batch(vg_ctx *ctx, const float *query, const float *targets, int64_t dim,
                            int64_t n, float *out, void *stream);
int32_t vg_dot_batch(vg_ctx *ctx, const float *query, const float *targets, int64_t dim,
                     int64_t n, float *out, void *stream);

/* simd.SquaredL2Bounded (kernels.go:173 -> bounded_l2_avx512.c:19-108), one query against n
 * contiguous targets with one bound each (bounds[n]) or a shared one (bounds[1], n_bounds=1).
 * (dist[i], exceeded[i]) = the pair the reference returns: the bounded kernel's reduction order run to completion
 * when the bound holds, and when it does not the PARTIAL total of the 64-float block at which the reference exits
 * (bounded_l2_avx512.c:60-75; an excess reached only in the 8-wide / scalar remainder returns the full sum). */
int32_t vg_squared_l2_bounded_batch(vg_ctx *ctx, const float *query, const float *targets, int64_t dim,
                                    int64_t n, const float *bounds, int64_t n_bounds, float *dist,
                                    int32_t *exceeded, void *stream);
/* simd.PqAdcLookup (kernels.go:56 -> pqAdcLookupAvx512, floats_avx512.c:135-167), batched:
 * one table (m*256 fp32, stride 256) against n codes of m bytes: out[n] */
int32_t vg_pq_adc_lookup_batch(vg_ctx *ctx, const float *table, const uint8_t *codes, int64_t m, int64_t n,
                               float *out, void *stream);

/* ---- internal/kmeans ------------------------------------------------------------------------- */
/* TrainKMeans kmeans.go:16-138: Lloyd on flat vectors[n*dim]; init = the first k entries of a
 * random permutation (seeded counter stream instead of the unseeded rand.Perm, kmeans.go:25),
 * assignment by SquaredL2Batch argmin (strict <) or DotBatch argmax (strict >) for Dot/Cosine,
 * update = index-ordered fp32 sums * (1/count), empty cluster -> random point, stop when no
 * assignment changed.  *produced = 0 and nothing written when n < k (the reference returns
 * (nil, nil), kmeans.go:17-20); metric Hamming -> VG_ERR_UNSUPPORTED. */
int32_t vg_kmeans_train(vg_ctx *ctx, const float *vectors, int64_t n, int32_t dim, int32_t k, int32_t metric,
                        int32_t max_iter, uint64_t seed, float *centroids, int32_t *produced, void *stream);
/* AssignPartition kmeans.go:142-196, batched: out[n] = index of the closest centroid */
int32_t vg_kmeans_assign(vg_ctx *ctx, const float *vectors, int64_t n, int32_t dim, const float *centroids,
                         int32_t k, int32_t metric, int32_t *out, void *stream);
/* FindClosestCentroids kmeans.go:217-280: the nprobe closest centroid indices for one query
 * (selection when nprobe <= k/4 && nprobe < 16, otherwise a sort by distance; ties by index).
 * Returns min(nprobe, k) indices in out; *n_out receives that count. */
int32_t vg_find_closest_centroids(vg_ctx *ctx, const float *query, const float *centroids, int32_t dim,
                                  int32_t k, int32_t nprobe, int32_t metric, int32_t *out, int32_t *n_out,
                                  void *stream);

/* ---- BinaryQuantizer (internal/quantization/binary.go) and NormalizeL2InPlace ------------------------
 * vg_binary_train   Train (:59-79): *threshold = float32(mean of every component, accumulated in float64).
 *                   The reference walks one float64 accumulator over the values in order; the device adds
 *                   float64 chunk sums, so the float32 result can differ by one ulp when the mean falls on
 *                   a rounding boundary (never observed) — the only entry point here that is not bit-exact.
 * vg_binary_encode  Encode / EncodeUint64Into (:86-154): bit i = (v[i] >= threshold), ceil(dim/64) little-
 *                   endian uint64 words per vector (threshold 0 = the sign bits RaBitQ stores).
 * vg_binary_decode  Decode (:173-188): threshold +- 0.5; code_bytes = bytes per code the caller holds
 *                   (bits beyond it read as 0).
 * vg_binary_hamming_batch   ComputeHammingDistance (:158-171) of one float query against n codes:
 *                   out[i] = popcount(encode(query) xor code_i) (HammingDistance :221-239 = simd.Hamming). */
int64_t vg_binary_code_bytes(int32_t dim);
int32_t vg_binary_train(vg_ctx *ctx, int32_t dim, const float *vectors, int64_t n, float *threshold, void *stream);
int32_t vg_binary_encode(vg_ctx *ctx, int32_t dim, float threshold, const float *vectors, int64_t n,
                         uint8_t *codes, void *stream);
int32_t vg_binary_decode(vg_ctx *ctx, int32_t dim, float threshold, const uint8_t *codes, int64_t n,
                         int32_t code_bytes, float *out, void *stream);
int32_t vg_binary_hamming_batch(vg_ctx *ctx, int32_t dim, float threshold, const float *query,
                                const uint8_t *codes, int64_t n, int32_t *out, void *stream);
/* distance.NormalizeL2InPlace (distance/distance.go:40-53) of n rows in place: norm2 = simd.Dot(v, v)
 * (dotProductAvx512 order), inv = 1 / simd.Sqrt(norm2) (float64 sqrt rounded to float32, float32 divide),
 * v[i] *= inv (scaleAvx512).  ok[row] (may be NULL) = 0 where the norm is zero (the row is left as it is —
 * the reference returns false) or dim == 0, else 1.  What cosine callers run before every insert / query
 * (engine/search.go:171-184, hnsw.go:799-818). */
int32_t vg_normalize_l2(vg_ctx *ctx, float *vectors, int64_t n, int32_t dim, uint8_t *ok, void *stream);

/* ---- searches ---------------------------------------------------------------- */
/* Segment.Rerank (flat/segment.go:754-780, diskann/segment.go:1093-1116,
 * engine/search.go:914-965): exact distance.SquaredL2 / distance.Dot
 * (squaredL2Avx512 / dotProductAvx512 order) of each query against its own nc
 * candidate rows, then the best k by (Score, RowID).  cand_ids[nq*nc] may hold
 * VG_INVALID_ID (skipped); a row listed twice is scored and reported twice, as in the reference's
 * loop.  k <= 512. */
int32_t vg_rerank(vg_index *idx, const float *queries, int64_t nq, const uint32_t *cand_ids,
                  int32_t nc, int32_t k, uint32_t *ids, float *scores, void *stream);
/* exact scores only, scores[nq*nc] in candidate order (invalid ids → +Inf / -Inf) */
int32_t vg_score_candidates(vg_index *idx, const float *queries, int64_t nq,
                            const uint32_t *cand_ids, int32_t nc, float *scores, void *stream);

/* flat.Segment.Search, fp32 branch (flat/segment.go:691-701) == exact brute force:
 * distance.SquaredL2 / distance.Dot of every row (squaredL2Avx512 / dotProductAvx512
 * order), best k by (Score, RowID) (segment.go:714-721).  (hnsw.BruteSearch, which keeps its results in a
 * PriorityQueue and reports HNSW distances, is vg_search_hnsw_brute.)  Candidates come from a batched query x base fp32 MFMA GEMM
 * (||x||^2 - 2 q.x); the survivors are re-scored in the reference's summation order and the
 * result is verified against the GEMM error bound (a query that fails the check is
 * recomputed by the exhaustive exact kernel), so ids and scores equal the reference's.
 * Metric L2 → ascending squared L2; Dot / Cosine → descending dot product
 * (distance.Provider, distance/distance.go:91-106).  k <= 512: up to k = 48 the 64 best GEMM
 * scores per query are re-scored and proved; above that every row under the query's threshold is
 * (the threshold is taken deeper in the sample for k > 64, ~3k rows pass it, sorted in LDS); batches
 * of up to 4 queries with k <= 64 take the exhaustive exact scan instead.
 * Above 128 queries (dim % 32 == 0, no bf16 filter) the candidates come from bfloat16 matrix products on the fp32 rows: up
 * to k = 16 first a SCREEN, one product of the operands' rounded halves with the bfloat16 rounding in the proof's margin, and
 * for the queries whose proof fails under that margin three products (fp32-grade margin) over their 256-query tiles only;
 * above k = 16 the three products for every query; then the exhaustive kernel as above.  vg_index_flat_retried counts the queries the screen left open. */
int32_t vg_search_flat(vg_index *idx, const float *queries, int64_t nq, int32_t k, uint32_t *ids,
                       float *scores, void *stream);
/* Optional bfloat16 FILTER for vg_search_flat (no reference counterpart; the results stay the reference's).  on != 0:
 * the index keeps a bfloat16 copy of its fp32 rows (n*dim*2 bytes more HBM, dim rounded up to a multiple of 64 with
 * zeros; made from the rows attached by vg_index_set_vectors, to be enabled again after the rows are replaced).  Searches
 * of more than 4 queries (smaller batches take the exact scan, which has no nomination step) then NOMINATE with
 * v_mfma_f32_32x32x16_bf16 over the copies instead of the fp32 MFMA GEMM; the nominated rows are re-scored from the fp32 rows in the reference's summation order exactly as without the filter,
 * and the proof that no other row can enter the top k widens its margin by what the rounding of the copies can change
 * (<= 2^-8 * 1.02 * (|q|^2 + max|x|^2)); a query whose proof fails goes to the exhaustive exact kernel as before.
 * Ids and scores are therefore bit-identical with and without the filter.  on == 0 drops the copy. */
int32_t vg_index_enable_bf16_filter(vg_index *idx, int32_t on, void *stream);

/* Engine.SearchThreshold over one flat segment (engine/engine.go:1485-1531): per query
 * flat.Segment.Search(q, k = max_results) (flat/segment.go:447-721, fp32 branch), then the rows with
 * Score <= thresholds[q] (L2) / Score >= thresholds[q] (Dot, Cosine) (:1518-1529), best first.
 * ids/scores[nq*max_results]; counts[nq] = rows kept; slots after counts[q] hold VG_INVALID_ID and
 * +Inf (L2) / -Inf (Dot, Cosine), as the other searches pad.  mask / mask_stride: the row filter,
 * with the same convention as vg_search_flat_filtered (NULL = none).  max_results <= 16384.
 * Both comparisons keep the boundary; a NaN threshold keeps nothing.  Up to 8 queries: an exact scan (one pass
 * over the rows) lists the rows within each threshold.  Larger batches: the fused GEMM of vg_search_flat (fp32, or
 * the bf16 filter when enabled) appends every row under the user's threshold widened by the GEMM's error bound, or
 * under a sampled threshold where that is lower; the appended rows are re-scored exactly and filtered, and a
 * query whose proof fails (list overflow, or a sampled threshold too close to its max_results-th score) is
 * answered by the scan.  Then the best max_results rows by (Score, RowID).  A query whose scores may hold a NaN
 * replays the reference's heap with k = max_results and filters what it pops.  nq == 0 or max_results == 0:
 * nothing is written.
 * VG_ERR_UNSUPPORTED: max_results > 16384, Hamming, an index with more than one IVF partition (the reference
 * would probe only nprobes of them).  Pointers may be host or device.  (VG_ABI_MINOR 11.) */
int32_t vg_search_flat_threshold(vg_index *idx, const float *queries, int64_t nq, const float *thresholds,
                                 int32_t max_results, const uint8_t *mask, int64_t mask_stride,
                                 uint32_t *ids, float *scores, int32_t *counts, void *stream);

/* diagnostics of vg_search_flat since vg_index_set_vectors: how many queries were searched and
 * how many of them were answered by the exhaustive kernel instead of GEMM candidates + proof
 * (either pointer may be NULL).  Synchronises the stream.  vg_search_flat_threshold counts alike: its
 * queries in the first count; in the second, the queries of a nominated batch whose proof failed and were
 * scanned (and every query under the test hook VG_FLAT_FORCE_EXACT).  Batches of up to 8 queries are scanned
 * from the start, like vg_search_flat's small batches, and are not counted in the second. */
int32_t vg_index_flat_stats(vg_index *idx, int64_t *queries, int64_t *exhaustive, void *stream);

/* one more count of vg_search_flat since vg_index_set_vectors: the queries whose one-product screen (see vg_search_flat) could
 * not prove their answer and which the three-product pass nominated again.  A retried query is not an exhaustive one: it counts
 * in vg_index_flat_stats' second value only if its second proof fails too.  Synchronises the stream. */
int32_t vg_index_flat_retried(vg_index *idx, int64_t *retried, void *stream);

/* and one more: the sum over the queries of vg_search_flat's GEMM path since vg_index_set_vectors of the candidates the nomination
 * appended to the query's list (a retried query: what its retry appended).  The thresholds come from a row sample; a wrong sample
 * gives no wrong answer but a slow one — thresholds too low show in vg_index_flat_stats' second value, thresholds too high here.
 * Found by symbol lookup, like vg_index_flat_retried.  Synchronises the stream. */
int32_t vg_index_flat_appended(vg_index *idx, int64_t *appended, void *stream);

/* exhaustive scan of the RaBitQ codes: RaBitQuantizer.Distance (rabitq.go:119-176) for every
 * row, best k by (Score, RowID).  The reference only scores RaBitQ codes node by node inside the
 * Vamana search (diskann/segment.go:512-535); the scan is the sharded config-5 workload
 * (SURVEY.md §8d).  k <= 512 (pages of 64 results, one scan per page). */
int32_t vg_search_rabitq(vg_index *idx, const float *queries, int64_t nq, int32_t k, uint32_t *ids,
                         float *scores, void *stream);

/* ---- SQ8 (internal/quantization/quantizer.go, internal/simd/src/sq8_avx512.c) ---------- */
/* NewScalarQuantizer quantizer.go:119-125 */
int32_t vg_sq8_create(vg_ctx *ctx, int32_t dim, vg_sq8 **out);
int32_t vg_sq8_destroy(vg_sq8 *sq);
int32_t vg_sq8_is_trained(vg_sq8 *sq);
/* Train quantizer.go:127-180: per-dimension min / max over vectors[n*dim]; a constant dimension
 * gets max = min + 1e-6; scale = 255 / range, invScale = range / 255 */
int32_t vg_sq8_train(vg_sq8 *sq, const float *vectors, int64_t n, void *stream);
/* SetBounds quantizer.go:52-78 (max - min < 1e-9 zeroes both scales) */
int32_t vg_sq8_set_bounds(vg_sq8 *sq, const float *mins, const float *maxs);
/* Mins / Maxs and the derived scales, dim floats each (any pointer may be NULL) */
int32_t vg_sq8_get_params(vg_sq8 *sq, float *mins, float *maxs, float *scales, float *inv_scales);
/* EncodeInto quantizer.go:198-222, batched: codes[n*dim] = uint8((clamp(v) - min) * scale + 0.5) */
int32_t vg_sq8_encode(vg_sq8 *sq, const float *vectors, int64_t n, uint8_t *codes, void *stream);
/* DecodeInto quantizer.go:240-250, batched: out[n*dim] = float32(code) * invScale + min */
int32_t vg_sq8_decode(vg_sq8 *sq, const uint8_t *codes, int64_t n, float *out, void *stream);
/* L2DistanceBatch quantizer.go:93-106 = simd.Sq8uL2BatchPerDimension in
 * sq8uL2BatchPerDimensionAvx512 order (sq8_avx512.c:59-103): out[n] */
int32_t vg_sq8_l2_distance_batch(vg_sq8 *sq, const float *query, const uint8_t *codes, int64_t n,
                                 float *out, void *stream);
/* codes[n*dim] in the reference's row-major layout (flat/segment.go s.codes); re-tiled on the
 * device for the scan.  The quantizer must outlive the index. */
int32_t vg_index_set_sq8_codes(vg_index *idx, vg_sq8 *sq, const uint8_t *codes, void *stream);
/* flat.Segment.Search, SQ8 branch: L2 segments score every row with L2DistanceBatch
 * (flat/segment.go:517-604), Dot / Cosine segments with ScalarQuantizer.DotProduct (:659-667,
 * quantizer.go:109-119: a sequential fp32 loop, largest first); best k by (Score, RowID).  k <= 512
 * (beyond 64 results the scan runs once per page of 64, each page after the previous one's last key). */
/* Optional bfloat16 NOMINATION for batches of vg_search_sq8 (no reference counterpart; the results stay the reference's).
 * on != 0: keeps the dequantised rows rounded to bfloat16 (rows * dim * 2 bytes, dim rounded up to a multiple of 64: twice
 * the codes) and their norms.  A batch of 5 or more queries (k <= 256) is then nominated by the bf16 MFMA GEMM of the flat
 * search, its 64 best rows per query (k > 48: every row below a sampled threshold) re-scored with L2Distance / DotProduct
 * (by the metric) from the CODES, and a bound on the nomination's error proves no other row can enter the k best; a query
 * whose proof fails is scanned as before.  Filtered batches over an unpartitioned segment (vg_search_flat_filtered,
 * VG_SCAN_SQ8) and partitions probed by 12 or more queries each (k <= 160, dim % 4 == 0) take it too.  Other shapes keep
 * the scan.  Dropped by vg_index_set_sq8_codes.  (VG_ABI_MINOR 9.) */
int32_t vg_index_enable_sq8_nomination(vg_index *idx, int32_t on, void *stream);
int32_t vg_search_sq8(vg_index *idx, const float *queries, int64_t nq, int32_t k, uint32_t *ids,
                      float *scores, void *stream);

/* ---- INT4 (internal/quantization/int4.go, internal/simd/src/int4_avx512.c) -------------- */
int32_t vg_int4_create(vg_ctx *ctx, int32_t dim, vg_int4 **out);
int32_t vg_int4_destroy(vg_int4 *iq);
int32_t vg_int4_is_trained(vg_int4 *iq);
/* Train int4.go:29-62: per-dimension min and diff = max - min (0 -> 1), then
 * simd.BuildInt4LookupTable (kernels.go:94-103) */
int32_t vg_int4_train(vg_int4 *iq, const float *vectors, int64_t n, void *stream);
/* UnmarshalBinary int4.go:190-219: min[dim], diff[dim] as stored, lookup table rebuilt */
int32_t vg_int4_set_params(vg_int4 *iq, const float *min_val, const float *diff);
/* min[dim], diff[dim], table[dim*16] (any pointer may be NULL) */
int32_t vg_int4_get_params(vg_int4 *iq, float *min_val, float *diff, float *table);
int64_t vg_int4_code_bytes(int32_t dim); /* (dim + 1) / 2 */
/* Encode int4.go:65-105, batched: two dimensions per byte, the even one in the high nibble,
 * quant = byte(math.Round(float64(clamp((v - min) / diff)) * 15)) */
int32_t vg_int4_encode(vg_int4 *iq, const float *vectors, int64_t n, uint8_t *codes, void *stream);
/* Decode int4.go:108-130, batched: float32(q)/15.0*diff + min */
int32_t vg_int4_decode(vg_int4 *iq, const uint8_t *codes, int64_t n, float *out, void *stream);
/* precomputed = 0: L2DistanceBatch (int4.go:150-164) = int4L2DistanceBatchAvx512 order
 * (int4_avx512.c:191-299); precomputed = 1: L2Distance (int4.go:133-147) =
 * int4L2DistancePrecomputedAvx512 order (:127-189) for each of the n codes.  out[n]. */
int32_t vg_int4_l2_distance_batch(vg_int4 *iq, const float *query, const uint8_t *codes, int64_t n,
                                  int32_t precomputed, float *out, void *stream);
/* Test entry point, read-only: what vg_int4_l2_distance_batch would launch for n > 0 rows whose codes are (1) or are not (0)
 * 16-byte aligned, on this context's device and under the test hook VG_INT4_SMALL_GRID as it stands.  Nothing runs.
 * plan[4] = {kernel, waves per workgroup, workgroups, dynamic LDS bytes}; kernel 0: the table scan (dim % 256 == 0, dim <= 1024),
 * 1: the pair-table scan over rows of whole 128-byte pieces, 2: the pair-table scan with a shorter last piece, 3: a lane per
 * row (dim % 64 != 0 or unaligned codes).  Both summation orders take the same plan.  Found by symbol lookup (see VG_ABI_MINOR). */
int32_t vg_int4_scan_plan(vg_int4 *iq, int64_t n, int32_t codes_aligned16, int64_t *plan);
/* INT4 codes of a DiskANN segment (diskann/segment.go:378-416), n * ceil(dim/2) bytes; scored by
 * vg_search_vamana kind 3.  The quantizer must outlive the index. */
int32_t vg_index_set_int4_codes(vg_index *idx, vg_int4 *iq, const uint8_t *codes, void *stream);
/* Exhaustive scan of the INT4 codes: Int4Quantizer.L2Distance (int4.go:136-147, int4L2DistancePrecomputedAvx512 order,
 * int4_avx512.c:127-189) for every row that takes part — the bits vg_int4_l2_distance_batch(precomputed = 1) writes for the row and
 * vg_search_vamana kind 3 reports for it.  The reference only scores INT4 codes node by node inside the Vamana search
 * (diskann/segment.go:558-565); the scan is the candidate stage of a rerank pipeline, the answer to a selective filter and the
 * walk's ground truth.  Scores ascend whatever the index's metric (the DiskANN scorer is this L2-type distance under every
 * metric, see vg_search_vamana_threshold).  ids / scores[nq * k]: the k best rows by (Score, RowID), best first; unused slots
 * VG_INVALID_ID / +Inf.  Pointers host or device, at any alignment.
 *   mask: the vg_search_vamana_filtered convention — bit i of byte i/8 set: row i takes part; query q reads mask + q * mask_stride,
 *   mask_stride 0: one mask for the batch, NULL: every row.  A 64-row tile none of whose rows a batch mask keeps is not read.
 *   k <= 512 (pages of 64 results, one scan per page).  Queries whose scores may hold a NaN are answered as
 *   flat.Segment.Search's heap loop answers them (flat/segment.go:714-721; "NaN scores" below).
 *   One query: the streaming scans of vg_int4_l2_distance_batch with the selection fused in (dim % 64 == 0; other dims a lane
 *   per row).  Batches of 5 queries or more: a workgroup carries 8 queries over every decoded row (dim % 32 == 0, dim <= 4096;
 *   other dims the lane-per-row kernel once per query — the same results, slower).  Nothing new is resident: the kernels read
 *   the index's own codes; per call the partial lists and the page state.
 *   Refusals, in this order, nothing written: NULL index VG_ERR_INVALID_ARG; negative nq or k VG_ERR_INVALID_ARG; nq == 0 or
 *   k == 0 VG_OK; rows but no INT4 codes VG_ERR_NOT_READY; NULL queries / ids / scores VG_ERR_INVALID_ARG; k > 512
 *   VG_ERR_UNSUPPORTED; mask_stride nonzero, nq > 1 and mask_stride < ceil(rows / 8) VG_ERR_INVALID_ARG.  An index without rows
 *   answers padding.  Found by symbol lookup (see VG_ABI_MINOR). */
int32_t vg_search_int4(vg_index *idx, const float *queries, int64_t nq, int32_t k, const uint8_t *mask, int64_t mask_stride,
                       uint32_t *ids, float *scores, void *stream);

/* ---- graph construction: neighbour selection ---------------------- */
/* Vamana robustPrune (diskann/writer.go:571-625) for n_nodes nodes at once.  cands[n_nodes*nc]
 * holds, per node, the search results and the node's current neighbours (what the reference's
 * `unique` map holds); VG_INVALID_ID entries, duplicates and the node itself are dropped.
 * Candidates are visited by ascending (distance to the node, id) — the reference's order among
 * equal distances is unspecified (map iteration + unstable sort) — and kept unless
 * alpha * dist(candidate, kept) < dist(candidate, node) for some already kept one.
 * out[n_nodes*r] (VG_INVALID_ID padded), counts[n_nodes].  nc <= 1024, r <= 256. */
int32_t vg_robust_prune(vg_index *idx, const uint32_t *nodes, int64_t n_nodes, const uint32_t *cands,
                        int32_t nc, int32_t r, float alpha, uint32_t *out, int32_t *counts, void *stream);
/* HNSW selectNeighborsHeuristic (hnsw.go:1009-1106: applyHeuristic + fillUpNeighbors; all the
 * candidates when there are at most m).  cand_ids / cand_dists[n_nodes*nc]: nearest first, with the
 * distance to the source as the caller's queue held it; lists may end in VG_INVALID_ID.
 * out[n_nodes*m], counts[n_nodes].  nc <= 1024, m <= 256. */
int32_t vg_hnsw_select_neighbors(vg_index *idx, int64_t n_nodes, const uint32_t *cand_ids,
                                 const float *cand_dists, int32_t nc, int32_t m, uint32_t *out,
                                 int32_t *counts, void *stream);

/* ---- IVF partitions of a flat segment (flat/segment.go:187-207, :727-749) ------------------- */
/* centroids[num_partitions*dim] and part_offsets[num_partitions+1] (first row of every partition,
 * non-decreasing, last <= rows) as the flat writer lays them out (rows grouped by partition).
 * num_partitions == 0 removes them. */
int32_t vg_index_set_partitions(vg_index *idx, const float *centroids, const uint32_t *part_offsets,
                                int32_t num_partitions, void *stream);
enum { VG_SCAN_F32 = 0, VG_SCAN_PQ = 1, VG_SCAN_SQ8 = 2 };
/* The partition-probed scan of flat.Segment.Search: per query kmeans.FindClosestCentroids(nprobes)
 * (kmeans.go:217-280; nprobes <= 0 means 1), then the chosen scan over those partitions' row ranges
 * only, one top-k by (score, row id).  With at most one partition it is vg_search_flat /
 * vg_search_pq_adc / vg_search_sq8.  k <= 512 (pages of 64 results), nprobes <= 64.  Equal centroid distances: the
 * reference's selection loop (kmeans.go:255-269, taken for nprobes <= partitions / 4 && nprobes < 16) is replayed, so the
 * probed partitions are the reference's also among duplicated centroids; its full sort leaves ties unpinned (by id here).
 * VG_SCAN_PQ takes any m: a table beyond one LDS image (m >= 144, e.g. dim 1536 at the writer's dim / 8 = 192) is walked in
 * 96 KiB chunks, same limits, same ids and score bits.  (An unpartitioned index is vg_search_pq_adc, whose k <= 64 for m > 96.) */
int32_t vg_search_flat_probed(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t nprobes,
                              int32_t scan, uint32_t *ids, float *scores, void *stream);
/* flat.Segment.Search with `filter segment.Filter` set (flat/segment.go:447): a row whose filter.Matches(rowID) is false
 * is skipped (fp32 / PQ rows before they are scored, :631-635; SQ8 L2 rows after their batch was scored, :559-561) — the
 * k best (score, row id) keys of the matching rows of the probed partitions, or of the whole segment when it has at most
 * one partition.  mask: bit i of byte i/8 set = filter.Matches(i) (tombstones are the caller's: clear their bits); query q
 * reads mask + q * mask_stride (0 = one mask for the batch, else >= ceil(rows/8)); NULL = vg_search_flat_probed.  Block
 * skipping by field statistics (MatchesBlock, :614-628) only ever skips rows no filter bit is set for.  k <= 512,
 * nprobes <= 64; VG_SCAN_PQ with any m, partitioned or not (a table beyond one LDS image is walked in chunks; a 64-row tile
 * the filter leaves nothing of is not read).  (VG_ABI_MINOR 4.) */
int32_t vg_search_flat_filtered(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t nprobes,
                                int32_t scan, const uint8_t *mask, int64_t mask_stride, uint32_t *ids, float *scores,
                                void *stream);

/* Engine.SearchThreshold (engine/engine.go:1485-1531) over a flat segment that carries codes and / or IVF partitions — what
 * vg_search_flat_threshold refuses.  Per query three steps:
 *   1. flat.Segment.Search(q, k = max_results, nprobes, filter) (flat/segment.go:447-751) with the scan `scan` (VG_SCAN_F32 fp32
 *      rows, VG_SCAN_SQ8 L2Distance / DotProduct of the codes by metric, VG_SCAN_PQ table lookups), over the whole segment or —
 *      more than one partition — the nprobes closest ones: the best max_results rows by (scan score, row id).  scan, nprobes,
 *      mask / mask_stride mean what they mean for vg_search_flat_filtered (nprobes <= 0 is 1, ignored with at most one
 *      partition, <= 64; NULL mask = none); probe choice and its tie rules are vg_search_flat_probed's; scan scores are bit for
 *      bit that entry's for the same row.
 *   2. rerank != 0: Segment.Rerank (flat/segment.go:754-780, engine/search.go:914-980) — every candidate's exact
 *      distance.SquaredL2 / distance.Dot from the index's fp32 rows, all of them ordered by (exact score, row id).  (With
 *      VG_SCAN_F32 the step changes nothing and is skipped.)
 *   3. the engine's filter (:1518-1529): Score <= thresholds[q] (L2) / Score >= thresholds[q] (Dot, Cosine), by the index's
 *      metric whatever the scan (a Dot / Cosine PQ scan keeps and compares its LARGEST table sums, as the reference's heap
 *      does).  The boundary is kept; NaN on either side keeps nothing.
 * rerank == 0 is the segment-level answer: the rows of step 1 whose SCAN score is within the threshold, scores the scan's.
 * rerank != 0 is the engine's: the threshold is compared with the exact score, scores are exact; needs fp32 rows on the index.
 * Output as vg_search_flat_threshold: ids/scores[nq*max_results], counts[nq], best first, the slots after counts[q] hold
 * VG_INVALID_ID and +Inf (L2) / -Inf (Dot, Cosine); host or device pointers; nq == 0 or max_results == 0 writes nothing.
 * Without rerank (and with fp32 rows either way) one scan appends the rows within the threshold to a list per query and the best
 * max_results of it are selected; with rerank over codes two scans find the best max_results rows by code score exactly (a
 * 65536-bin histogram of the keys' top 16 bits per query, then every key at or below the bin where the count reaches
 * max_results), which are re-scored, filtered and ordered.  The whole segment is read once per 8 queries (PQ: per query), a
 * probed partition once per (query, probe) pair.
 * NaN scores: a query whose scan scores may hold a NaN or an Inf has step 1 answered by the reference's heap replayed with
 * k = max_results over the same ranges (see "NaN scores"); steps 2 and 3 follow the replay.  Not restated, as for vg_rerank:
 * NaN EXACT scores inside step 2's heap are dropped by the filter and the rest are ordered by key.
 * Refusals, each decided before any work: max_results > 16384 VG_ERR_UNSUPPORTED (the number in the message); Hamming
 * VG_ERR_UNSUPPORTED; nprobes > 64 VG_ERR_UNSUPPORTED; a scan kind the index has no data for, or rerank != 0 without fp32
 * rows, VG_ERR_NOT_READY; a PQ of other than 256 centroids VG_ERR_UNSUPPORTED, as vg_search_flat_probed(VG_SCAN_PQ).  A PQ
 * table that does not fit one LDS image (m > 96) is served: its scan walks the table in 96 KiB chunks for 32 tiles of rows at a
 * time, the same scores, lists and passes.  (Present when the symbol is: see VG_ABI_MINOR.) */
int32_t vg_search_flat_probed_threshold(vg_index *idx, const float *queries, int64_t nq, const float *thresholds,
                                        int32_t max_results, int32_t nprobes, int32_t scan /* VG_SCAN_* */, int32_t rerank,
                                        const uint8_t *mask, int64_t mask_stride,
                                        uint32_t *ids, float *scores, int32_t *counts, void *stream);

/* flat.Writer.Flush's partitioning and quantization (flat/writer.go:99-223) on the resident index, over its fp32 rows where
 * they lie.  (Present when the symbol is: see VG_ABI_MINOR.)
 * Partitioning (:105-169), skipped when num_partitions <= 1 or rows < num_partitions (the index then has 0 partitions and
 *   perm is the identity): kmeans.TrainKMeans over all rows with the index's metric = vg_kmeans_train(seed), kmeans_iters
 *   iterations (0 = the writer's 10, :109), the centroids bit for bit; AssignPartition per row = vg_kmeans_assign; then the
 *   writer's counting sort (:132-153): partition p's rows start at the exclusive prefix sum of the counts and keep their
 *   ascending original order — exactly a stable sort by partition, part_offsets[P] = rows, an empty partition is two equal
 *   offsets.  perm[new] = old and inv_perm[old] = new, either NULL to skip, host or device.  The rows, their norms and the
 *   bf16 filter image move into that order; centroids and offsets are attached as vg_index_set_partitions attaches them.  The
 *   caller permutes what the index never held: ids, metadata, payloads.
 * Quantization (:171-223) of the reordered rows: VG_QUANT_NONE; VG_QUANT_SQ8: vg_sq8_train + vg_sq8_encode with `sq`, attached
 *   as vg_index_set_sq8_codes does; VG_QUANT_PQ: `pq` = vg_pq_create(dim, pq_m, 256), pq_m 0 = dim / 8 (:66), vg_pq_train with
 *   pq_iters iterations (0 = 20) and the same seed, vg_pq_encode, attached as vg_index_set_pq_codes does.  The quantizers are
 *   the caller's objects, trained by this call, and outlive it like any quantizer an index refers to.
 * Refusals, in this order, with nothing changed and nothing written: NULL index VG_ERR_INVALID_ARG; no fp32 rows
 *   VG_ERR_NOT_READY; metric Hamming VG_ERR_UNSUPPORTED; an HNSW or Vamana graph, codes of any kind, partitions or a
 *   nomination image already on the index VG_ERR_UNSUPPORTED; an unknown quantization, negative counts, or a kind without its
 *   quantizer VG_ERR_INVALID_ARG; a quantizer of another dimension VG_ERR_DIM_MISMATCH; a vg_pq that is not (pq_m, 256)
 *   VG_ERR_INVALID_ARG; a PQ shape vg_pq_train refuses: its status.  rows == 0 is VG_OK with nothing done.
 * Memory: one scratch buffer of the rows' size while they move, O(rows) for the order, the codes once more before they are
 *   attached; released before the call returns. */
int32_t vg_flat_build(vg_index *idx, int32_t num_partitions, int32_t quantization, int32_t pq_m, int32_t kmeans_iters,
                      int32_t pq_iters, uint64_t seed, vg_sq8 *sq, vg_pq *pq, uint32_t *perm, uint32_t *inv_perm, void *stream);

/* ---- on-disk segment images --------------------------------------- */
enum { VG_QUANT_NONE = 0, VG_QUANT_PQ = 1, VG_QUANT_SQ8 = 3, VG_QUANT_RABITQ = 5, VG_QUANT_INT4 = 6 }; /* quantization.Type, types.go:6-14 */
typedef struct vg_segment_info {
    uint64_t segment_id;
    int64_t rows;
    int32_t dim, metric;
    int32_t kind;          /* 0 = flat segment, 1 = DiskANN segment */
    int32_t quantization;  /* VG_QUANT_* */
    int32_t pq_m, pq_k;
    int32_t max_degree, search_list_size; /* DiskANN R and L (diskann/format.go:26-27) */
    uint32_t entrypoint;
    int32_t num_partitions; /* flat segment: IVF partitions (flat/format.go:37) */
} vg_segment_info;
/* flat.Open (flat/segment.go:105-300) over a whole segment file held in host memory (mmap or
 * read): header (flat/format.go:11-165), optional CRC32C of the body, SQ8 bounds / PQ codebooks,
 * codes and fp32 rows are uploaded as they lie in the file.  The result owns a vg_index (and the
 * quantizer the file describes); search it with vg_search_flat / vg_search_sq8 / vg_search_pq_adc
 * / vg_rerank.  Errors carry the reference's messages ("invalid magic number", "unsupported
 * version", "file too short for vectors", "checksum mismatch: ..."). */
int32_t vg_segment_open_flat(vg_ctx *ctx, const void *image, int64_t size, int32_t verify_checksum,
                             vg_segment **out, void *stream);
/* flat.Segment.Search (flat/segment.go:447-751, filter == nil) for a batch of queries: the scan type
 * follows the segment (SQ8 codes: L2Distance / DotProduct by metric; PQ: table lookups, L2 segments
 * only — see vg_segment.hip; else fp32 rows) and, when the segment has more than one IVF partition,
 * only the nprobes closest partitions are scanned (:727-744; nprobes <= 0 means 1).  k <= 512 and
 * nprobes <= 64 on the partitioned path.  A PQ segment of any m is searched, filtered and threshold-searched
 * (vg_segment_search_filtered, vg_segment_search_threshold); only the unpartitioned, unfiltered search of a
 * table beyond one LDS image (m > 96) keeps vg_search_pq_adc's k <= 64.
 * On a DiskANN segment: diskann.Segment.Search (diskann/segment.go:487-706) = vg_search_vamana with
 * the distFn of the segment's quantization (RaBitQ, else PQ, else INT4, else fp32); nprobes is unused,
 * like the search-list size the reference computes and never reads. */
int32_t vg_segment_search(vg_segment *seg, const float *queries, int64_t nq, int32_t k, int32_t nprobes,
                          uint32_t *ids, float *scores, void *stream);
/* Segment.Search with `filter` set, by what the file holds: vg_search_flat_filtered (flat/segment.go:631-635) or
 * vg_search_vamana_filtered (diskann/segment.go:616-627).  mask: bit i of byte i/8 = filter.Matches(i), query q's at
 * mask + q * mask_stride (0 = one for the batch); NULL = vg_segment_search.  (VG_ABI_MINOR 8.) */
int32_t vg_segment_search_filtered(vg_segment *seg, const float *queries, int64_t nq, int32_t k, int32_t nprobes,
                                   const uint8_t *mask, int64_t mask_stride, uint32_t *ids, float *scores, void *stream);
/* Engine.SearchThreshold over one segment, by what the file holds: a flat segment is vg_search_flat_probed_threshold with the
 * scan vg_segment_search picks (SQ8 codes, else PQ, else fp32 rows); a DiskANN segment is vg_search_vamana_threshold with the
 * segment's kind — nprobes and rerank are ignored there (the walk's scores are what the engine compares).
 * (Present when the symbol is: see VG_ABI_MINOR.) */
int32_t vg_segment_search_threshold(vg_segment *seg, const float *queries, int64_t nq, const float *thresholds,
                                    int32_t max_results, int32_t nprobes, int32_t rerank, const uint8_t *mask,
                                    int64_t mask_stride, uint32_t *ids, float *scores, int32_t *counts, void *stream);
/* diskann segment (diskann/format.go:8-119, segment.go:165-440,1393-1408): fp32 rows, the
 * N x R uint32 graph and entry point, PQ codebooks + codes or RaBitQ codes; search with
 * or INT4 parameters + codes; search with vg_search_vamana (kind 0 / 1 / 2 / 3).  The header's
 * CompressionType byte is ignored exactly as segment.go ignores it: the reference writer records
 * LZ4 there by default (writer.go:92) while writing every section raw (writer.go:697-740). */
int32_t vg_segment_open_diskann(vg_ctx *ctx, const void *image, int64_t size, int32_t verify_checksum,
                                vg_segment **out, void *stream);
int32_t vg_segment_get_info(vg_segment *seg, vg_segment_info *info);
vg_index *vg_segment_index(vg_segment *seg); /* borrowed: valid until vg_segment_close */
vg_pq *vg_segment_pq(vg_segment *seg);       /* NULL unless the segment is PQ-quantized */
vg_sq8 *vg_segment_sq8(vg_segment *seg);     /* NULL unless the segment is SQ8-quantized */
vg_int4 *vg_segment_int4(vg_segment *seg);   /* NULL unless the segment is INT4-quantized */
int32_t vg_segment_close(vg_segment *seg);
/* hash.CRC32C (internal/hash/crc32c.go:15-17) */
uint32_t vg_crc32c(const void *data, int64_t size);
/* The same over `size` bytes of DEVICE memory, computed there: any start address, any length.  *out = the CRC (0 for
 * size 0).  Status: NULL context / result / data, a negative size or host memory VG_ERR_INVALID_ARG.  (See VG_ABI_MINOR.) */
int32_t vg_crc32c_device(vg_ctx *ctx, const void *device_ptr, int64_t size, uint32_t *out, void *stream);
/* The file flat.Writer.Flush writes (flat/writer.go:312-470) for the resident index, into a host buffer: the 152-byte header
 * (flat/format.go:28-56, :112-133), then with NO padding between them the centroids, the partition offsets, the quantization
 * metadata (SQ8: mins then maxs; PQ: u32 m, u32 256, scales, offsets, int8 codebooks), the codes row-major, the fp32 rows,
 * the ids as little-endian uint64, the metadata section and the block statistics.  Every header offset is the running
 * position (:335-345), also of a section that is absent; NumPartitions is 0 for an unpartitioned index; Checksum is the
 * CRC-32C of everything behind the header, the codes' and rows' share computed on the device (vg_crc32c_device) while the host
 * checksums the small sections.  The payload side file is the host's.
 *   ids: rows values in the index's (new) row order, NULL = 0 .. rows-1.
 *   metadata_section / block_stats: the host's serialisation (:230-307) of its documents, permuted like the ids, copied
 *     verbatim; NULL = what the writer emits when no row has a document: rows + 1 zero uint32 offsets and no blob; block
 *     statistics uvarint(ceil(rows / 1024)) then per block uvarint(1), 0x00; for rows == 0 no metadata section and the one
 *     byte 0x00.  vg_segment_flat_image_size takes the two sizes, a negative one standing for that NULL form.
 *   *written (may be NULL) = vg_segment_flat_image_size = the bytes written.
 * vg_segment_flat_image_size touches no device and changes nothing; -1 where vg_segment_write_flat would refuse the index.
 * Refusals: a NULL index or image, image_size below vg_segment_flat_image_size VG_ERR_INVALID_ARG; rows > 0 without fp32
 *   rows VG_ERR_NOT_READY; a graph on the index, RaBitQ or INT4 codes (the flat format has no type for them, format.go:22-26),
 *   SQ8 and PQ codes at once, a PQ of other than 256 centroids VG_ERR_UNSUPPORTED.  (See VG_ABI_MINOR.) */
int64_t vg_segment_flat_image_size(const vg_index *idx, int64_t metadata_bytes, int64_t block_stats_bytes);
int32_t vg_segment_write_flat(vg_index *idx, uint64_t segment_id, const uint64_t *ids, const void *metadata_section,
                              int64_t metadata_bytes, const void *block_stats, int64_t block_stats_bytes, void *image,
                              int64_t image_size, int64_t *written, void *stream);

/* diskann.Writer.Write up to Flush (diskann/writer.go:217-253) on the resident index, over its fp32 rows where they lie, in the
 * writer's order.  (Present when the symbol is: see VG_ABI_MINOR.)
 * 1. Quantize (:229-242, :274-360) the rows in add order: VG_QUANT_NONE; VG_QUANT_PQ with `pq` = vg_pq_create(dim, pq_m, 256):
 *    trainPQ's rule first — fewer than 256 rows switch quantization off (:276-279: *quantization_used = VG_QUANT_NONE, `pq`
 *    untouched, no codes; 256 rows train) — else vg_pq_train with pq_iters iterations (0 = 20) and `seed`, vg_pq_encode,
 *    attached as vg_index_set_pq_codes does; VG_QUANT_RABITQ: vg_rabitq_encode, attached as vg_index_set_rabitq_codes does;
 *    VG_QUANT_INT4 with `iq`: vg_int4_train + vg_int4_encode, attached as vg_index_set_int4_codes does.  The quantizers are the
 *    caller's objects, trained by this call, and outlive it like any quantizer an index refers to.
 * 2. buildGraph (:244-247) = vg_vamana_build(idx, r, l, alpha, NULL, seed, max_batch, growth_div): its defaults and limits.
 * 2.5 reorderBFS (:249-253) = vg_vamana_reorder_bfs(idx, perm, inv_perm): either may be NULL, host or device; the codes of
 *    step 1 move with the rows.  The caller permutes what the index never held: ids, metadata, payloads.
 * The result is bit for bit what those calls give when made one after another.  *quantization_used (may be NULL) = the
 *   VG_QUANT_* kind of the codes that ended up on the index.
 * Refusals, in this order, with nothing changed and nothing written: NULL index VG_ERR_INVALID_ARG; rows without fp32 rows
 *   VG_ERR_NOT_READY; rows == 0 VG_ERR_INVALID_ARG ("no vectors to write", :218-220); codes of any kind, IVF partitions, a
 *   Vamana graph, a nomination image, an HNSW graph or its tombstones or edge distances VG_ERR_UNSUPPORTED; an unknown
 *   quantization, VG_QUANT_SQ8 (the DiskANN format has none) or a kind without its quantizer VG_ERR_INVALID_ARG; VG_QUANT_PQ with
 *   pq_m <= 0 VG_ERR_INVALID_ARG (a deviation: the reference then trains nothing, :230, and writes a header that claims PQ with
 *   no codes behind it, :678-681); a vg_pq that is not (pq_m, 256) VG_ERR_INVALID_ARG; a quantizer of another dimension
 *   VG_ERR_DIM_MISMATCH; then what vg_pq_train (when it will train), vg_index_set_rabitq_codes and vg_vamana_build refuse about
 *   the shape, with their own status and message.
 * A failure after these checks (out of memory, a HIP error) returns its status with *quantization_used, perm and inv_perm
 *   unwritten, and leaves the index at the step it reached: a failure in step 1 leaves no codes attached (the quantizer may be
 *   trained); in step 2 the codes of step 1 in add order and no graph; in step 2.5 codes and graph in add order when the
 *   failure is an allocation (vg_vamana_reorder_bfs allocates before it moves anything), while after a HIP error in its
 *   permutation the per-row arrays may disagree and the index is only good for vg_index_destroy. */
int32_t vg_diskann_build(vg_index *idx, int32_t r, int32_t l, float alpha, int32_t quantization, int32_t pq_m, int32_t pq_iters,
                         uint64_t seed, int32_t max_batch, int32_t growth_div, vg_pq *pq, vg_int4 *iq, uint32_t *perm,
                         uint32_t *inv_perm, int32_t *quantization_used, void *stream);
/* The file diskann.Writer.Flush writes (diskann/writer.go:645-856) for the resident index, into a host buffer: the 160-byte
 * header (diskann/format.go:51-78), then with NO padding between them (bytesWritten is a running sum, :695-833) the fp32 rows,
 * the graph (rows x MaxDegree little-endian uint32, VG_INVALID_ID = empty slot: the resident table verbatim), the codes
 * row-major with their parameters behind them, the ids as little-endian uint64, the metadata section and the metadata
 * inverted index.  Codes: PQ at PQCodesOffset, then at PQCodebookOffset m fp32 scales, m fp32 offsets and the int8 codebooks
 * (no `m, K` in front, unlike the flat format, :742-763); INT4 at PQCodesOffset, then at PQCodebookOffset
 * Int4Quantizer.MarshalBinary (quantization/int4.go:171-188: u32 dim, min[dim], diff[dim]), which ends where the ids start;
 * RaBitQ at BQCodesOffset, no parameters.
 *   Header: Magic 0x4449534B, Version 2, SegmentID, RowCount, Dim, Metric; MaxDegree = the graph's r; SearchListSize =
 *     search_list_size (the index does not keep l; 0 = NewWriter's 100); Entrypoint = the index's; QuantizationType = the
 *     VG_QUANT_* kind of the codes on the index; PQSubvectors / PQCentroids for PQ, else 0; CompressionType = compression_type
 *     verbatim (0, 1 or 2: the reference records 1 = LZ4 by default, :92, and writes every section raw, :697-740, as this call
 *     does); padding and reserved bytes 0.  Offsets of absent sections stay 0 (they are assigned inside their branches only,
 *     :727-775) and BlockStatsOffset is 0, the writer never sets it.  Checksum = CRC-32C of everything behind the header: the
 *     rows', graph's and codes' share computed on the device and chained on the host, which checksums the small sections.
 *   ids: rows values in the index's (new) row order, NULL = 0 .. rows-1.
 *   metadata_section: the host's serialisation (:797-823) of its documents permuted like the ids, copied verbatim; NULL = rows + 1
 *     zero uint64 offsets and no blob.  metadata_index: WriteInvertedIndex's bytes (:825-833), verbatim; NULL = the one byte
 *     0x00 of an empty index (internal/metadata/unified.go:1724-1733).  vg_segment_diskann_image_size takes the two sizes, a
 *     negative one standing for that NULL form.  The payload side file stays the host's.
 *   *written (may be NULL) = vg_segment_diskann_image_size = the bytes written.
 * vg_segment_diskann_image_size touches no device and changes nothing; -1 where vg_segment_write_diskann would refuse the index.
 * Refusals, in this order, with nothing written: a NULL index or image, a compression_type outside 0..2, a negative
 *   search_list_size or a negative size of a given section VG_ERR_INVALID_ARG; rows == 0 VG_ERR_INVALID_ARG; no fp32 rows or no
 *   Vamana graph VG_ERR_NOT_READY; an HNSW graph, IVF partitions, SQ8 codes or more than one kind of codes VG_ERR_UNSUPPORTED;
 *   image_size below vg_segment_diskann_image_size VG_ERR_INVALID_ARG.  (See VG_ABI_MINOR.) */
int64_t vg_segment_diskann_image_size(const vg_index *idx, int64_t metadata_bytes, int64_t metadata_index_bytes);
int32_t vg_segment_write_diskann(vg_index *idx, uint64_t segment_id, int32_t search_list_size, int32_t compression_type,
                                 const uint64_t *ids, const void *metadata_section, int64_t metadata_bytes,
                                 const void *metadata_index, int64_t metadata_index_bytes, void *image, int64_t image_size,
                                 int64_t *written, void *stream);

/* per-query counters, the reference's FilterGateStats (searcher/searcher.go:114-137).  vg_search_vamana has
 * no short-circuit path; it reports in distance_short_circuits the candidates it could NOT push because the
 * per-query exploration heap (min(rows, 65536) entries for k <= 512 unfiltered, rows otherwise; the reference's is unbounded) was full — 0 in every
 * search that followed the reference exactly. */
typedef struct vg_search_stats {
    int64_t nodes_visited, distance_computations, distance_short_circuits, pops;
    /* not a FilterGateStats field: rows scored by greedySearch on the way down through the upper layers
     * (hnsw.go:1897-1934 does not count them) — part of a query's gathered bytes all the same */
    int64_t descent_distance_computations;
} vg_search_stats;

/* hnsw.KNNSearch (hnsw.go:1650-1755): greedySearch through the upper layers (:1897-1934), then
 * searchLayerUnfiltered on layer 0 (:1220-1396) with the reference's exact heap semantics
 * (searcher/queue.go 4-ary heaps: bounded result heap of ef, exploration heap capped at 2*ef with
 * the adaptive shrink, strict comparisons), distance.SquaredL2Bounded short-circuit
 * (bounded_l2_avx512.c order) once ef results exist, distFunc otherwise (L2 / -Dot / 0.5*L2:
 * vectorstore/columnar.go:29-50).  One wavefront per query, many queries in flight; per query
 * the result equals the sequential reference's.  ids/scores[nq*k] best first; stats[nq] may be
 * NULL.  k <= ef (a smaller ef is raised to k, determineEF hnsw.go:1891-1894); the two heaps of a query live
 * in LDS up to ef = 512 and in HBM scratch beyond.  NaN distances (a NaN or an Inf in a row or in a query): every
 * comparison with a NaN is false in the reference (queue.go:75-82,199-203, hnsw.go:1376), and the result is the
 * reference's here too — a walk that scores a NaN stops and the query is answered by a second pass that compares
 * floats exactly as the reference's loop is written (r04 and before: unspecified, and an Inf in a query could fault). */
int32_t vg_search_hnsw(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t ef,
                       uint32_t *ids, float *scores, vg_search_stats *stats, void *stream);
/* searchExecute with a filter and a selectivity hint above highSelectivityThreshold = 0.3 (hnsw.go:1107-1146, :1791-1835):
 * searchLayerWithPostFilter (hnsw.go:1159-1218) — the walk above with ef expanded to ef * (1 + (1 - selectivity) / 2)
 * (at most 2 ef, at most 500), every result then popped worst first, the rows whose mask bit is set kept in that order and
 * pushed back capped at ef — and knnSearchInternal's extraction.  mask: bit i of byte i/8 set = row i passes
 * (filter.Matches and not tombstoned); query q reads mask + q * mask_stride (0 = one mask for the batch, else >=
 * ceil(n/8)).  `ef` is what determineEF returned (its bitmap-cardinality expansion, hnsw.go:1863-1889, is the caller's).
 * selectivity <= 0.3 (0 = no hint): the reference walks predicate-aware there — vg_search_hnsw_predicate below with no
 * tombstones (VG_ABI_MINOR 6; before it this returned VG_ERR_UNSUPPORTED).  (VG_ABI_MINOR 3.) */
int32_t vg_search_hnsw_filtered(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t ef,
                                const uint8_t *mask, int64_t mask_stride, double selectivity, uint32_t *ids,
                                float *scores, vg_search_stats *stats, void *stream);
/* searchExecute with a filter and a selectivity hint at or below 0.3, or none: searchLayerPredicateAware (hnsw.go:1406-1558) on
 * layer 0 — per neighbour, in list order: filter.Matches and the tombstone bit BEFORE any distance; a passing live node is
 * scored; a rejected one is navigated by its cached edge distance (Neighbor.Dist > 0, node.go:62-80) while the results hold
 * fewer than ef/2 items, scored while they hold fewer than ef unless more than 10 rejections came in a row or its edge
 * distance exceeds 1.5 x the worst result, and skipped once they hold ef; the navigation queue is unbounded, the results are
 * bounded by ef and take passing live nodes only; then knnSearchInternal's extraction.  mask as above (filter.Matches only);
 * deleted: the tombstone bitmap, one for the batch, NULL = none.  stats: nodes_visited, distance_computations,
 * distance_short_circuits = ExpansionsSkipped, pops.  ef <= 4096.  fp32 rows.  Needs the layer-0 edge distances:
 * vg_index_set_hnsw_edge_distances, else they are recomputed from the rows at the first call.  (VG_ABI_MINOR 6.) */
int32_t vg_search_hnsw_predicate(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t ef,
                                 const uint8_t *mask, int64_t mask_stride, const uint8_t *deleted, uint32_t *ids,
                                 float *scores, vg_search_stats *stats, void *stream);
/* The cached Neighbor.Dist of the layer-0 lists, l0_dist[n*m0] slot for slot with vg_index_set_hnsw_graph's l0 (the low 32
 * bits of the reference's neighbour words, node.go:67-80); NULL = recompute them from the fp32 rows as the distance between
 * the two nodes, which is what the insert stored (hnsw.go:516, :550, :964).  Dropped when the graph is replaced. */
int32_t vg_index_set_hnsw_edge_distances(vg_index *idx, const float *l0_dist, void *stream);
/* g.tombstones (hnsw.go:95, Delete :1601-1617) as a bitmap: bit i of byte i/8 set = node i deleted, ceil(n/8) bytes; NULL = no
 * deleted node.  A deleted node is walked through but never enters the results, so it never moves the bound either
 * (searchLayerUnfiltered hnsw.go:1381-1390, processEntryPointUnfiltered :1559-1565, the post-filter's re-filter :1198,
 * searchLayerPredicateAware :1485, :1580).  Read by vg_search_hnsw, _hnsw_pq, _hnsw_filtered and — when its own `deleted`
 * argument is NULL — vg_search_hnsw_predicate; while it is set the unfiltered / post-filter walks run as the pass that
 * compares as the reference writes it (the one that answers NaN distances), somewhat slower than the tuned walk.
 * vg_search_hnsw_brute takes the tombstones inside its mask, as before.  (VG_ABI_MINOR 7.) */
int32_t vg_index_set_hnsw_tombstones(vg_index *idx, const uint8_t *deleted, void *stream);
/* The same walk scored from the nodes' PQ codes instead of their fp32 rows: distFunc =
 * pq.ComputeAsymmetricDistance (pq.go:234-260), the way the reference scores graph nodes from PQ codes
 * (diskann/segment.go:536-557); no SquaredL2Bounded short-circuit (that kernel reads fp32 rows).  scores =
 * the PQ distances.  Candidate stage of graph -> PQ -> exact rerank (engine/search.go:914-965): ask for
 * k = ef candidates, then vg_rerank.  Needs vg_index_set_pq_codes (numCentroids 256) and metric L2. */
int32_t vg_search_hnsw_pq(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t ef,
                          uint32_t *ids, float *scores, vg_search_stats *stats, void *stream);

/* diskann.Segment.searchInternal (diskann/segment.go:503-706), filters nil.  kind selects the
 * distFn: 0 = fp32 rows (distance.Provider(metric), :582-588), 1 = PQ
 * ComputeAsymmetricDistance (:536-541, terms summed sequentially over the sub-quantizers),
 * 2 = RaBitQ Distance (:512-519), 3 = INT4 L2Distance (:558-565).  Unbounded exploration
 * min-heap, top-k CandidateHeap,
 * stop when the popped candidate is worse than the k-th result.  k <= 16384; k is the only knob of how far the walk goes
 * (RefineFactor's searchK = k * RefineFactor, engine/search.go:192, and SearchThreshold's maxResults reach it as k).
 * k <= 512 runs the kernels it always ran (the k best in registers, or a sorted LDS list above 64; exploration heap of
 * min(rows, 65536) items).  512 < k <= 16384: the k best are a 64-ary max-heap of (score, id) keys (the top 449 in LDS,
 * the rest in HBM), the exploration heap holds every row (nothing is ever dropped), and the k keys are sorted once at the
 * end; a query whose scores may hold a NaN replays CandidateHeap with k items in LDS.  Same ids, score bits, order and
 * counters as the reference at every k.  k > 16384: VG_ERR_UNSUPPORTED. */
int32_t vg_search_vamana(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t kind,
                         uint32_t *ids, float *scores, vg_search_stats *stats, void *stream);
/* The same with `filter segment.Filter` set: pushToHeap (diskann/segment.go:616-627) returns before TryPushBounded for a row
 * whose filter.Matches is false — the traversal queue still takes the node, and the stop test reads the heap of MATCHING rows,
 * so a selective filter walks further before it stops.  mask: bit i of byte i/8 set = filter.Matches(i) (and the metadata
 * filter, :620-622, if any — the host ANDs them); query q reads mask + q * mask_stride (0 = one mask for the batch, else >=
 * ceil(rows/8)); NULL = vg_search_vamana.  (VG_ABI_MINOR 5.) */
int32_t vg_search_vamana_filtered(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t kind,
                                  const uint8_t *mask, int64_t mask_stride, uint32_t *ids, float *scores,
                                  vg_search_stats *stats, void *stream);
/* FreshVamana.Search (fresh_vamana.go:272-315) and, with a mask, SearchWithFilter (:318-364) over the index's Vamana graph
 * and fp32 rows.  greedySearch (:535-613) is the walk of vg_vamana_insert's step 1 with caps 2 ef and ef, except that results
 * takes every node, deleted ones too.  l = FreshVamana's search list size (0 = 100); only ef is limited.
 *   mask NULL: ef = max(2k, l); the first k results that are not deleted are returned.
 *   mask set:  ef = max(10k, 2l); the first k results that are not deleted and whose mask bit is set.  mask / mask_stride as
 *     for vg_search_vamana_filtered (bit i of byte i/8 = filter(i), query q's at mask + q * mask_stride, 0 = one for the batch).
 *   deleted: as for vg_vamana_insert, ceil(n/8) bytes, NULL = none.
 * ids / scores: nq * k, scores the walk's distances (vg_vamana_insert's Distance and NaN rules); counts[q] <= k rows found
 * (may be NULL), the remaining slots hold VG_INVALID_ID and +Inf (L2) / -Inf (Dot, Cosine) as the threshold searches pad
 * them.  An index without rows answers counts 0.  ef > 2048 (two lists of 2 ef and ef 8-byte keys, ping-ponged in LDS)
 * VG_ERR_UNSUPPORTED; no graph VG_ERR_NOT_READY.  Pointers may be host or device.  (Present when the symbol is: see
 * VG_ABI_MINOR.) */
int32_t vg_search_vamana_fresh(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t l, const uint8_t *deleted,
                               const uint8_t *mask, int64_t mask_stride, uint32_t *ids, float *scores, int32_t *counts,
                               void *stream);
/* Engine.SearchThreshold's DiskANN leg (engine/engine.go:1485-1531): per query vg_search_vamana_filtered(q, k =
 * max_results) — the walk runs with the full k, the threshold prunes nothing — then the engine's filter (:1518-1529):
 * Score <= thresholds[q] for L2, Score >= thresholds[q] for Dot and Cosine, by the index's metric even for the code scorers
 * (whose scores are L2-type distances), as the engine compares.  The boundary is kept; a NaN threshold keeps nothing, a NaN
 * score is dropped.  The kept rows stay in walk order, compacted to the front; counts[q] = rows kept; the other slots hold
 * VG_INVALID_ID and +Inf (L2) / -Inf (Dot, Cosine).  thresholds: one per query; mask / mask_stride as for
 * vg_search_vamana_filtered (NULL = none); stats as for vg_search_vamana (may be NULL).  nq == 0 or max_results == 0:
 * nothing is written.  max_results > 16384: VG_ERR_UNSUPPORTED.  Pointers may be host or device.  (Present when the symbol is: see VG_ABI_MINOR.) */
int32_t vg_search_vamana_threshold(vg_index *idx, const float *queries, int64_t nq, const float *thresholds,
                                   int32_t max_results, int32_t kind, const uint8_t *mask, int64_t mask_stride,
                                   uint32_t *ids, float *scores, int32_t *counts, vg_search_stats *stats, void *stream);

/* The HNSW index's two EXHAUSTIVE paths, each with the heap it is written with (searcher/queue.go) — which ids
 * survive a tie at the k-th distance and the order of equal distances in the result follow from the heap's layout,
 * so the heap is replayed operation by operation (vg_search_flat / vg_rerank order by (Score, RowID) instead, the
 * CandidateHeap order of flat/segment.go:714-721, and report dot products; this entry reports HNSW distances):
 *   VG_BRUTE_SCAN    hnsw.BruteSearch + scanSegment (hnsw.go:2021-2101): PriorityQueue(max); len < k -> PushItem,
 *                    else `d < top.Distance` -> PopItem + PushItem; res[len-1 .. 0] = PopItem().
 *   VG_BRUTE_BITMAP  searchBitmap (hnsw.go:2240-2263) + knnSearchInternal's extraction (:1732-1751):
 *                    s.Candidates.TryPushBounded(item, k) (at capacity `d >= top` is rejected, else the item replaces
 *                    the root and sifts down); popped, reversed.
 * Rows are visited in ascending id (node segments in order; bm.ForEach ascending, segment/segment.go:154).  mask: bit i
 * of byte i/8 set = row i takes part — for SCAN the rows that are live nodes and pass `filter`, for BITMAP the
 * bitmap minus the tombstones; NULL = every row.  Query q reads mask + q*mask_stride (mask_stride 0 = one mask for
 * the batch, else >= ceil(n/8)).  Distances as the index wraps them (hnsw.go:2218-2238, columnar.go:37-44): L2 ->
 * squared L2, Dot -> -dot, Cosine -> 0.5 * squared L2 (rows and queries normalised by the caller, as for
 * vg_search_hnsw).  ids/scores[nq*k] best first; unused slots VG_INVALID_ID / +Inf.  k <= 1024.  NaN distances (a NaN
 * or Inf in a row or query; dot products overflowing both ways) are answered as the reference's loops answer them — `d <
 * top.Distance` never admits a NaN once the heap is full, `d >= top.Distance` never rejects one — by a pass that decides every
 * row against the live top (r05 and before: unspecified; see "NaN scores" below). */
enum { VG_BRUTE_SCAN = 0, VG_BRUTE_BITMAP = 1 };
int32_t vg_search_hnsw_brute(vg_index *idx, const float *queries, int64_t nq, int32_t k, int32_t mode,
                             const uint8_t *mask, int64_t mask_stride, uint32_t *ids, float *scores, void *stream);

/* engine fan-in (engine/search.go:904-908: per-segment candidate lists merged into one
 * bounded heap, ordered by searcher/candidate_queue.go:12-23).  Here the "segments" are row
 * shards, one per GPU: lists[l] holds nq*k (id, score) results of shard l, ids local to the
 * shard; id_offsets[l] (may be NULL = all 0) is added to make them global.  Output: the k best
 * of the union per query, best first.  metric picks the direction (L2 ascending, Dot/Cosine
 * descending).  ids_in/scores_in are [lists][nq][k] contiguous; every list best first, unused slots
 * VG_INVALID_ID at its end.  k <= 1024.
 * A candidate that repeats across lists — the same score and the same GLOBAL id in two lists: replicated
 * or overlapping shards with id_offsets NULL, or offsets that make two ids coincide — is kept as often as
 * it is listed, the copies adjacent, as the engine's heap keeps candidates that differ only in SegmentID;
 * the merge does not deduplicate.  Zero scores of opposite sign are equal (InternalCandidateBetter
 * compares floats): among them the lower global id comes first, whatever the sign, and every score is
 * returned with the sign it came with (see "NaN scores": such a query is answered by the fan-in replay).
 * id_offsets are expected to ascend with the list, so that (SegmentID, RowID) orders like the global id. */
int32_t vg_merge_topk(vg_ctx *ctx, const uint32_t *ids_in, const float *scores_in, int32_t lists,
                      int64_t nq, int32_t k, int32_t metric, const uint32_t *id_offsets,
                      uint32_t *ids, float *scores, void *stream);
/* The same merge over the all-gathered image of vg_comm_all_gather_topk: packed[lists][2][nq][k] uint32 in
 * device memory, [l][0] = ids of list l, [l][1] = the bit patterns of its fp32 scores. */
int32_t vg_merge_topk_packed(vg_ctx *ctx, const uint32_t *packed, int32_t lists, int64_t nq, int32_t k,
                             int32_t metric, const uint32_t *id_offsets, uint32_t *ids, float *scores,
                             void *stream);

/* ---- multi-GPU: the one exchange step of a row-sharded search --------------------------------------
 * One process (or OS thread) per GPU, each with its own vg_ctx and its shard of the rows resident
 * (rows are independent, ids are global row numbers).  The reference merges per-segment
 * candidate lists into one bounded heap in-process (engine/search.go:835-908); here the lists cross GPUs:
 * ONE ncclAllGather (RCCL over xGMI) of nq*k*8 bytes per rank on the caller's stream, then vg_merge_topk
 * with the reference's tie-break on every rank.  RCCL is dlopen'ed on first use.
 *   vg_comm_unique_id   rank 0 fills id[VG_COMM_ID_BYTES] (ncclGetUniqueId); the host hands the bytes to
 *                       the other ranks by whatever channel it has (Go: a pipe, a file, its RPC layer)
 *   vg_comm_create      collective: every rank calls it with the same id (ncclCommInitRank)
 *   vg_comm_all_gather_topk   local_ids / local_scores [nq*k] = this rank's vg_search_* output (local row
 *                       numbers), id_offsets[world] = first global row of every shard; ids / scores [nq*k]
 *                       = the merged global top-k, identical on every rank
 *   vg_comm_all_gather  raw bytes (device buffers): e.g. the codebooks of a PQ trained by sub-quantizer
 *                       ranges (vg_pq_train_subset + vg_pq_get_codebooks_range) */
#define VG_COMM_ID_BYTES 128
typedef struct vg_comm vg_comm;
int32_t vg_comm_unique_id(uint8_t *id);
int32_t vg_comm_create(vg_ctx *ctx, int32_t world, int32_t rank, const uint8_t *id, vg_comm **out);
int32_t vg_comm_destroy(vg_comm *comm);
int32_t vg_comm_info(const vg_comm *comm, int32_t *world, int32_t *rank);
/* vg_comm_probe: load RCCL without creating anything (NOT a collective): every rank calls it and the host agrees on
 * the outcome BEFORE any rank enters vg_comm_create, which is a collective (ncclCommInitRank) — a rank that cannot
 * load RCCL would otherwise leave its peers waiting inside it.  An RCCL that is already mapped into the process (e.g.
 * PyTorch's torch/lib/librccl.so) is reused, never a second copy; rccl_path receives the file the symbols came from.
 * vg_comm_describe: what RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice), for the run's record: a line that claims n_gpus = N should carry rccl_ranks = N. */
int32_t vg_comm_probe(char *rccl_path, int32_t len);
int32_t vg_comm_describe(const vg_comm *comm, int32_t *rccl_ranks, int32_t *rccl_rank, int32_t *rccl_device,
                         int32_t *reused_mapped_rccl, char *rccl_path, int32_t len);
int32_t vg_comm_all_gather(vg_comm *comm, const void *send, void *recv, int64_t bytes_per_rank, void *stream);
int32_t vg_comm_all_gather_topk(vg_comm *comm, const uint32_t *local_ids, const float *local_scores,
                                int64_t nq, int32_t k, int32_t metric, const uint32_t *id_offsets,
                                uint32_t *ids, float *scores, void *stream);

/* NaN scores in the exhaustive searches and the beam search (vg_search_flat, vg_search_pq_adc, vg_search_sq8, vg_search_rabitq,
 * vg_search_flat_probed / _filtered, vg_search_hnsw_brute, vg_search_vamana / _filtered; VG_ABI_MINOR 10).  The scans keep their best k by a 64-bit key (score
 * bits, row id) — a total order, which is what the reference's heaps implement while no score is a NaN.  For a NaN every
 * comparison of candidate_queue.go:12-38 / queue.go:75-82,199-203 is false: a NaN that enters while the heap fills stays, at
 * the root it is never replaced (rows better than everything kept are turned away), as a first child it stops a sift.  That
 * outcome is DEFINED — the loops are sequential — and these entry points return it: a query whose INPUTS could produce a NaN
 * or an infinite score (a non-finite query value; non-finite rows, quantizer parameters or stored norms; magnitudes whose
 * partial sums can overflow: dim * max|q| * max|x| >= 1e38 for dot products, dim * (max|q| + max|x|)^2 >= 1e38 for squared
 * distances; RaBitQ: 4 |q| |y| >= 1e38 — +Inf scores are ties the heap breaks by row id inside its history, which the scans'
 * `score < bound` pre-tests do not reproduce while the bound is +Inf) is answered a second time by the reference's
 * heap replayed operation by operation with float comparisons, rows in the reference's order, and overwrites the first answer.
 * ids / scores then hold what the engine takes out of the heap — Pop() until empty (engine/search.go:859-862) — best first; a
 * NaN score's sign and payload are the instruction set's, not the algorithm's.  (vg_search_flat_prefilter replays the engine's OWN loop,
 * search.go:717-733: the same test, but `Pop(); Push(c)` at capacity where flat/segment.go:719 does ReplaceTop — with a NaN in the
 * heap the two leave different layouts and, later, different answers.)  Rare by construction (such inputs are garbage)
 * and slow by design: one workgroup walks all rows per query — measured at 1M x 768 (tools/nan_replay_time.py): a call of 1024
 * queries takes 11.6 ms with none at risk, 90 ms with one, 101 ms with 64, 698 ms with all of them; an index holding a non-finite
 * row sends EVERY query there.  Every other query pays one extra kernel launch per call that returns at once (the probed searches: two —
 * the probe lists are selected again for the replay).  vg_search_flat_probed / vg_search_flat_filtered (and vg_segment_search
 * through them) take part: the rows a query's filter lets through, the probed partitions' ranges in FindClosestCentroids'
 * order — its selection loop and, up to 12 partitions, its full sort (Go's insertion sort, where a NaN distance compares equal
 * to everything) are replayed; with more than 12 partitions AND NaN centroid distances the full sort is pdqsort proper, whose
 * order is not restated (NaN distances sort last).  vg_merge_topk / _packed (and vg_comm_all_gather_topk through them) replay
 * the engine's fan-in (engine/search.go:904-918: every list from its last valid entry to its first into one heap with
 * TryPushBounded, then popped) for a query whose lists hold a NaN.  The same fan-in replay also answers a query whose lists hold
 * a -0.0 score: the key orders -0.0 strictly before +0.0, the reference's float comparison ties them.  Not covered: vg_rerank — the order in which the engine hands
 * it the candidates comes out of an unstable sort (search.go:921), so there is no defined outcome to reproduce; NaN scores
 * order as the largest keys there. */

/* flat.Segment.Search, PQ branch (flat/segment.go:476-483 LUT, :678-689 ADC
 * = simd.PqAdcLookup in pqAdcLookupAvx512 order, :714-721 top-k with the
 * (Score, RowID) tie-break of searcher/candidate_queue.go:12-23).
 * queries[nq*dim] → ids[nq*k], scores[nq*k], best first.  k <= 1024. */
int32_t vg_search_pq_adc(vg_index *idx, const float *queries, int64_t nq, int32_t k,
                         uint32_t *ids, float *scores, void *stream);
/* Optional bfloat16 NOMINATION for batches of vg_search_pq_adc (no reference counterpart; the results stay the reference's).
 * A row's table sum is the squared distance to its DECODED vector (ProductQuantizer.Decode, pq.go:185-229: the table's
 * entries, pq.go:468-491, are computed from the same fp32 centroid values).  on != 0 keeps the decoded rows rounded to
 * bfloat16 (rows * dim * 2 bytes, dim rounded up to a multiple of 64 — 2 * dim / m times the codes: 16x at 8 dimensions per
 * sub-quantizer) and their norms.  A batch of queries x rows >= 24M (k <= 256, numCentroids == 256) is then nominated by the
 * bf16 MFMA GEMM of the flat search, its 64 best rows per query (k > 48: every row below a sampled threshold) re-scored
 * from the CODES against the query's BuildDistanceTable in pqAdcLookupAvx512 order, and a bound on the nomination's error
 * proves no other row can enter the k best; a query whose proof fails is scanned as before.  Smaller batches and the
 * filtered / probed searches keep the table scan.  Dropped by vg_index_set_pq_codes.  (VG_ABI_MINOR 10.) */
int32_t vg_index_enable_pq_nomination(vg_index *idx, int32_t on, void *stream);
/* The same nomination WITHOUT the image of the decoded rows, for the index sizes PQ exists for.  With 8 dimensions per
 * sub-quantizer a 16-byte granule of a decoded bfloat16 row is exactly one centroid, so the nomination GEMM fills its row tiles
 * from a bfloat16 copy of the decoded codebook ((dim padded to 64) / 8 * 4 KiB: 393 KB at m = 96, resident in the L2) by the row's
 * code bytes; the operands are bit for bit the image's, and so are the re-score, the proof and the results.  Resident: that
 * codebook, the rows' norms (4 bytes a row) and their largest — at most rows * (4 + dim_pad / 32) + (dim_pad / 8 + 1) * 4096 + 4096
 * bytes, 0.05x the codes at m = 96 where the image is 16x; the threshold sample's row tiles (rows / 64) are decoded into the call's
 * scratch.  Refusals as vg_index_enable_pq_nomination's, in its order (NULL index, no PQ codes, untrained, numCentroids != 256),
 * then sub-vectors of other than 8 dimensions: VG_ERR_UNSUPPORTED.  Any m (granules from m on read zeros).  The two modes
 * are exclusive: enabling one frees the other's state; on == 0 frees this one's; vg_index_set_pq_codes drops it.  Batches it takes:
 * unfiltered, ascending, k <= 256, rows > k, 16-byte aligned device queries, MORE THAN 128 queries, and queries x rows at or above
 * its own crossover against the scan (README, Limits); every other batch keeps the table scan, with the same results.  Found by
 * symbol lookup. */
int32_t vg_index_enable_pq_nomination_from_codes(vg_index *idx, int32_t on, void *stream);
/* Which PQ nomination an index holds and what it costs: *mode = 0 (off), 1 (the image: vg_index_enable_pq_nomination) or 2 (from
 * the codes); *held_bytes = the device memory the mode keeps resident (mode 1: the image, the norms and norm_max).  Either
 * pointer may be NULL.  Found by symbol lookup. */
int32_t vg_index_pq_nomination_info(const vg_index *idx, int32_t *mode, int64_t *held_bytes);
/* vg_index_enable_sq8_nomination WITHOUT the image of the dequantised rows.  A code is an integer, and bfloat16 holds c - 128
 * exactly: the nomination GEMM multiplies the queries scaled by the inverse scales, bf16(q_d * inv_d) — the only rounded operand —
 * by the centred codes, which its row tiles convert from the index's own code tiles; its scores differ from the image mode's by the
 * per-query constant 2 q.mid (Dot: q.mid), mid_d = min_d + 128 inv_d, which the proof takes back.  Re-score (sq.L2Distance /
 * sq.DotProduct on the codes), proof and results are the image mode's and the scan's, bit for bit.  Resident: the rows' norms
 * (4 bytes a row), mid (4 bytes a padded dimension) and two floats — rows * 4 + dim_pad * 4 + 8 bytes, where the image is rows *
 * dim_pad * 2; the threshold sample's row tiles (rows / 64) are converted into the call's scratch.  Refusals as
 * vg_index_enable_sq8_nomination's (NULL index, no SQ8 codes).  The two modes are exclusive: enabling one frees the other's
 * state; on == 0 frees this one's and leaves the other; vg_index_set_sq8_codes drops either.  Batches it takes: whole-segment
 * vg_search_sq8, L2 or Dot, unfiltered, MORE THAN 128 queries, k <= 256, rows > k, 16-byte aligned device queries, and queries x
 * rows at or above its crossover against the scan (README, Limits); filtered batches, probed partitions and smaller batches keep
 * the scan, with the same results.  Found by symbol lookup. */
int32_t vg_index_enable_sq8_nomination_from_codes(vg_index *idx, int32_t on, void *stream);
/* Which SQ8 nomination an index holds and what it does: *mode = 0 (off), 1 (the image: vg_index_enable_sq8_nomination) or 2 (from
 * the codes); *held_bytes = the device memory the mode keeps resident; *rescanned = the queries, since the mode was enabled, whose
 * proof failed and which the scan answered (0 when off).  Any pointer may be NULL.  Found by symbol lookup. */
int32_t vg_index_sq8_nomination_info(const vg_index *idx, int32_t *mode, int64_t *held_bytes, int64_t *rescanned);
/* vg_search_rabitq batches through an int8 matrix-core nomination.  A Hamming distance is a dot product of +-1 vectors: the GEMM
 * multiplies the queries' and rows' sign bits, expanded to int8 in registers from the index's own code tiles, and accumulates in
 * int32 — the Hamming distance of every (query, row) pair comes out EXACT, no rounded operand and no margin.  Its epilogue lists
 * (row, h) for the pairs whose exact score may be at or below the query's threshold (the sel-th best score of every 64th 64-row
 * tile): a conservative screen — every pair whose rq.Distance, in the reference's operation order, is <= the threshold passes —
 * that replaces the formula's division by a product with RN(1 / dim) moved one ulp towards zero (below 1 / dim, so the product
 * rounds to no more than the quotient).  The listed rows are re-scored with popcount and the reference's formula, the k best taken by (score, row id), and a
 * query is proved when its list (4096 keys) did not overflow and holds k rows at or below the threshold; the others go through the
 * scan.  Results are the scan's, bit for bit; the NaN replay stays the last step.  Resident: nothing beyond the code tiles and
 * norms (held_bytes 0).  The screen's inequality needs stored norms that are not negative (Encode's never are): enabling looks at
 * them once, and an index that holds a NEGATIVE stored norm keeps the scan for every batch.  Refusals: NULL index
 * VG_ERR_INVALID_ARG; no RaBitQ codes VG_ERR_NOT_READY.  on == 0 turns the mode off; vg_index_set_rabitq_codes drops it; enabling
 * again zeroes the counters; vg_vamana_reorder_bfs leaves it correct (nothing of it is per row).  Batches it takes: MORE THAN 128
 * queries, k <= 256, rows > k, any dim the index accepts, and queries x rows at or above its crossover against the scan (README,
 * Limits); every other batch runs the scan as before.  Found by symbol lookup. */
int32_t vg_index_enable_rabitq_nomination(vg_index *idx, int32_t on, void *stream);
/* *on = whether the mode is enabled; *held_bytes = the device memory it keeps resident (0); *rescanned = the queries, since the mode
 * was enabled, whose list was incomplete and which the scan answered; *mismatched = under the test hook VG_RABITQ_NOM_CHECK, the
 * listed keys whose Hamming distance from the GEMM was not the popcount's (0 unless the kernel is wrong).  Zeros when off.  Any
 * pointer may be NULL.  Found by symbol lookup. */
int32_t vg_index_rabitq_nomination_info(const vg_index *idx, int32_t *on, int64_t *held_bytes, int64_t *rescanned, int64_t *mismatched);

#ifdef __cplusplus
}
#endif
#endif /* VECGO_HIP_H */
