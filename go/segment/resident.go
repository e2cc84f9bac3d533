//go:build hip && cgo

// Package segment (HIP twin): a device-resident copy of one segment — what flat.Segment.Search
// (internal/segment/flat/segment.go:447-749), the DiskANN beam search (diskann/segment.go:503-706), the memtable's
// hnsw.KNNSearch (hnsw.go:1650-1755) and Segment.Rerank (flat/segment.go:754-780) run against, ONE call per query
// batch instead of one distance call per candidate.  filter == nil paths only: metadata filters and tombstones stay
// on the Go side.
//
// Ownership: Upload* copy the slices to HBM and retain nothing; results are written into caller-owned slices;
// Close frees the device memory.
package segment

/*
#cgo CFLAGS: -I${SRCDIR}/../../third_party/vecgo_hip/include
#cgo LDFLAGS: -L${SRCDIR}/../../third_party/vecgo_hip -lvecgo_hip
#include <stdlib.h>
#include "vecgo_hip.h"
*/
import "C"

import (
	"fmt"
	"unsafe"

	"github.com/hupe1980/vecgo/distance"
	"github.com/hupe1980/vecgo/internal/hipctx"
)

// Stats mirrors vg_search_stats = the reference's FilterGateStats counters (searcher/searcher.go:114-137) plus
// the rows the greedy descent scored.  Its size is part of the ABI (VG_ABI_VERSION).
type Stats struct {
	NodesVisited, DistanceComputations, DistanceShortCircuits, Pops int64
	DescentDistanceComputations                                    int64
}

const (
	ScanF32 = int32(C.VG_SCAN_F32)
	ScanPQ  = int32(C.VG_SCAN_PQ)
	ScanSQ8 = int32(C.VG_SCAN_SQ8)
)

// Vamana node scorers (diskann/segment.go:512-589 distFn).
const (
	VamanaF32, VamanaPQ, VamanaRaBitQ, VamanaInt4 = 0, 1, 2, 3
)

type Resident struct {
	ctx  *C.vg_ctx
	h    *C.vg_index
	seg  *C.vg_segment // set when opened from a segment image
	rows int
	dim  int
}

func fp(p []float32) *C.float  { return (*C.float)(unsafe.Pointer(&p[0])) }
func up(p []uint32) *C.uint32_t { return (*C.uint32_t)(unsafe.Pointer(&p[0])) }
func bp(p []byte) *C.uint8_t    { return (*C.uint8_t)(unsafe.Pointer(&p[0])) }
func ip(p []int32) *C.int32_t   { return (*C.int32_t)(unsafe.Pointer(&p[0])) }

// NewResident creates an empty twin of a segment of `rows` x `dim`.
func NewResident(rows, dim int, metric distance.Metric) (*Resident, error) {
	p, err := hipctx.Ptr()
	if err != nil {
		return nil, err
	}
	r := &Resident{ctx: (*C.vg_ctx)(p), rows: rows, dim: dim}
	if st := C.vg_index_create(r.ctx, C.int64_t(rows), C.int32_t(dim), C.int32_t(metric), &r.h); st != C.VG_OK {
		return nil, hipctx.Err(int32(st))
	}
	return r, nil
}

// OpenFlat / OpenDiskANN hand a whole segment file (mmap or read) to the library: header, section bounds and —
// with verify — the CRC32C are checked as flat.Open / diskann Open check them (flat/segment.go:105-300,
// diskann/segment.go:165-440); the sections are uploaded as they lie in the file.
func OpenFlat(image []byte, verify bool) (*Resident, error)    { return open(image, verify, false) }
func OpenDiskANN(image []byte, verify bool) (*Resident, error) { return open(image, verify, true) }

func open(image []byte, verify, diskann bool) (*Resident, error) {
	p, err := hipctx.Ptr()
	if err != nil {
		return nil, err
	}
	r := &Resident{ctx: (*C.vg_ctx)(p)}
	v := C.int32_t(0)
	if verify {
		v = 1
	}
	var st C.int32_t
	if diskann {
		st = C.vg_segment_open_diskann(r.ctx, unsafe.Pointer(&image[0]), C.int64_t(len(image)), v, &r.seg, nil)
	} else {
		st = C.vg_segment_open_flat(r.ctx, unsafe.Pointer(&image[0]), C.int64_t(len(image)), v, &r.seg, nil)
	}
	if st != C.VG_OK {
		return nil, hipctx.Err(int32(st)) // "invalid magic number", "checksum mismatch: ...", "file too short for ..."
	}
	var info C.vg_segment_info
	if st := C.vg_segment_get_info(r.seg, &info); st != C.VG_OK {
		C.vg_segment_close(r.seg)
		return nil, hipctx.Err(int32(st))
	}
	r.h = C.vg_segment_index(r.seg) // borrowed: lives until vg_segment_close
	r.rows, r.dim = int(info.rows), int(info.dim)
	return r, nil
}

func (r *Resident) Close() {
	if r.seg != nil {
		C.vg_segment_close(r.seg)
	} else if r.h != nil {
		C.vg_index_destroy(r.h)
	}
	r.seg, r.h = nil, nil
}

// ---- uploads (the reference's in-memory layouts, copied) ---------------------------------------------------------

// UploadVectors: one n*dim row-major array (vectorstore/columnar.go:21-24, flat/segment.go:692).
func (r *Resident) UploadVectors(base []float32) error {
	return hipctx.Err(int32(C.vg_index_set_vectors(r.h, fp(base), nil)))
}

// UploadPQCodes: n*m code bytes (flat/segment.go:678-680) scored with the quantizer behind `pq`
// (HIPProductQuantizer.Handle()).
func (r *Resident) UploadPQCodes(pq unsafe.Pointer, codes []byte) error {
	return hipctx.Err(int32(C.vg_index_set_pq_codes(r.h, (*C.vg_pq)(pq), bp(codes), nil)))
}

// UploadSQ8Codes: n*dim code bytes (flat/segment.go:550) with the quantizer behind `sq`.
func (r *Resident) UploadSQ8Codes(sq unsafe.Pointer, codes []byte) error {
	return hipctx.Err(int32(C.vg_index_set_sq8_codes(r.h, (*C.vg_sq8)(sq), bp(codes), nil)))
}

// UploadInt4Codes: n*ceil(dim/2) code bytes (diskann/segment.go:378-416).
func (r *Resident) UploadInt4Codes(iq unsafe.Pointer, codes []byte) error {
	return hipctx.Err(int32(C.vg_index_set_int4_codes(r.h, (*C.vg_int4)(iq), bp(codes), nil)))
}

// UploadRaBitQCodes: n*BytesTotal() code bytes (diskann/segment.go:1393-1408).
func (r *Resident) UploadRaBitQCodes(codes []byte) error {
	return hipctx.Err(int32(C.vg_index_set_rabitq_codes(r.h, bp(codes), nil)))
}

// UploadPartitions: IVF centroids and the first row of every partition (flat/segment.go:727-749).
func (r *Resident) UploadPartitions(centroids []float32, partitionOffsets []uint32, numPartitions int) error {
	return hipctx.Err(int32(C.vg_index_set_partitions(r.h, fp(centroids), up(partitionOffsets), C.int32_t(numPartitions), nil)))
}

// UploadVamanaGraph: n*R neighbour ids, 0xFFFFFFFF = none (diskann/segment.go:1376-1391).
func (r *Resident) UploadVamanaGraph(R int, graph []uint32, entry uint32) error {
	return hipctx.Err(int32(C.vg_index_set_vamana_graph(r.h, C.int32_t(R), up(graph), C.uint32_t(entry), nil)))
}

// UploadHNSWGraph: layer 0 as n*m0 ids; the upper layers as per-level slot tables and adjacency rows.
func (r *Resident) UploadHNSWGraph(m0 int, l0 []uint32, maxLevel, m int, upperSlot, upperAdj []uint32, levelRows []int64, entry uint32) error {
	var slot, adj *C.uint32_t
	var lr *C.int64_t
	if maxLevel > 0 {
		slot, adj, lr = up(upperSlot), up(upperAdj), (*C.int64_t)(unsafe.Pointer(&levelRows[0]))
	}
	return hipctx.Err(int32(C.vg_index_set_hnsw_graph(r.h, C.int32_t(m0), up(l0), C.int32_t(maxLevel), C.int32_t(m), slot, adj, lr,
		C.uint32_t(entry), nil)))
}

// BuildHNSW: ApplyBatchInsert over the rows (hnsw.go:639-684): ids = row numbers, levels = layerForApplyInsert.
func (r *Resident) BuildHNSW(m, efConstruction int) error {
	return hipctx.Err(int32(C.vg_hnsw_build(r.h, C.int32_t(m), C.int32_t(efConstruction), 8192, 32, nil)))
}

// InsertHNSW: hnsw.ApplyInsert for len(rows)/dim new rows (hnsw.go:629-637), appended as rows r.rows.. and linked
// into the resident HNSW graph (vg_hnsw_insert).  On an empty Resident the first call creates the rows and the graph.
func (r *Resident) InsertHNSW(rows []float32, m, efConstruction int) error {
	if r.dim <= 0 || len(rows)%r.dim != 0 {
		return fmt.Errorf("segment: InsertHNSW: %d floats are not whole rows of %d", len(rows), r.dim)
	}
	count := len(rows) / r.dim
	if count == 0 {
		return nil
	}
	if err := hipctx.Err(int32(C.vg_hnsw_insert(r.h, fp(rows), C.int64_t(count), C.int32_t(m), C.int32_t(efConstruction), 8192, 32, nil))); err != nil {
		return err
	}
	r.rows += count
	return nil
}

// CompactHNSW: hnsw.Compact (internal/hnsw/compact.go:16-34) on the resident graph under its tombstones
// (vg_hnsw_compact): live nodes with mostly dead lists are repaired, dead ids leave the live nodes' lists, dead nodes'
// lists are emptied.  The tombstones stay set; a tombstoned entry point is the caller's to re-elect (recoverEntryPoint).
func (r *Resident) CompactHNSW(efConstruction int) error {
	return hipctx.Err(int32(C.vg_hnsw_compact(r.h, C.int32_t(efConstruction), 8192, nil, nil)))
}

// BuildVamana: diskann.Writer.buildGraph over the rows (diskann/writer.go:362-460) with the seeded initial graph;
// R, L, alpha of 0 take NewWriter's defaults.  The graph replaces the resident Vamana graph.
func (r *Resident) BuildVamana(R, L int, alpha float32, seed uint64) error {
	return hipctx.Err(int32(C.vg_vamana_build(r.h, C.int32_t(R), C.int32_t(L), C.float(alpha), nil, C.uint64_t(seed), 8192, 32, nil)))
}

// InsertVamana: FreshVamana.Insert for len(rows)/dim new rows (diskann/fresh_vamana.go:178-222), appended as rows r.rows..
// and linked into the resident Vamana graph (vg_vamana_insert).  R, L, alpha of 0 take FreshDefault*.  deleted: bit i of byte
// i/8 = node i is deleted (FreshVamana.Delete; the rows before the call), nil = none.  On an empty Resident the first call
// creates the rows and the graph.
func (r *Resident) InsertVamana(rows []float32, R, L int, alpha float32, deleted []byte, seed uint64) error {
	if r.dim <= 0 || len(rows)%r.dim != 0 {
		return fmt.Errorf("segment: InsertVamana: %d floats are not whole rows of %d", len(rows), r.dim)
	}
	count := len(rows) / r.dim
	if count == 0 {
		return nil
	}
	var dp *C.uint8_t
	if deleted != nil {
		if len(deleted) < (r.rows+7)/8 {
			return fmt.Errorf("segment: InsertVamana: deleted holds %d bytes, %d needed", len(deleted), (r.rows+7)/8)
		}
		if len(deleted) > 0 {
			dp = bp(deleted)
		}
	}
	if err := hipctx.Err(int32(C.vg_vamana_insert(r.h, fp(rows), C.int64_t(count), C.int32_t(R), C.int32_t(L), C.float(alpha), dp, C.uint64_t(seed), 8192, 32, nil))); err != nil {
		return err
	}
	r.rows += count
	return nil
}

// ConsolidateVamana: FreshVamana.consolidate (diskann/fresh_vamana.go:803-867) on the resident Vamana graph
// (vg_vamana_consolidate): every live node that lists a deleted one gets a new list from a fresh search and prune; no
// reverse edges, the entry point stays.  L, alpha of 0 take FreshDefault*.  deleted as for InsertVamana, over all r.rows
// rows; nil = nothing to do.  The host keeps the bitmap and the trigger (more than a tenth of the nodes deleted).
func (r *Resident) ConsolidateVamana(L int, alpha float32, deleted []byte) error {
	var dp *C.uint8_t
	if deleted != nil {
		if len(deleted) < (r.rows+7)/8 {
			return fmt.Errorf("segment: ConsolidateVamana: deleted holds %d bytes, %d needed", len(deleted), (r.rows+7)/8)
		}
		if len(deleted) > 0 {
			dp = bp(deleted)
		}
	}
	return hipctx.Err(int32(C.vg_vamana_consolidate(r.h, C.int32_t(L), C.float(alpha), dp, 8192, nil, nil)))
}

// ReorderVamanaBFS: diskann.Writer.reorderBFS (diskann/reorder.go:14-157) on the resident graph and every per-row array
// it holds.  perm[new] = old; invPerm[old] = new is the writer's addOrderToFinalRow.  The caller permutes what the GPU
// never held (ids, metadata, payloads) with perm.
func (r *Resident) ReorderVamanaBFS() (perm, invPerm []uint32, err error) {
	perm, invPerm = make([]uint32, r.rows), make([]uint32, r.rows)
	if r.rows == 0 {
		return perm, invPerm, hipctx.Err(int32(C.vg_vamana_reorder_bfs(r.h, nil, nil, nil)))
	}
	if err := hipctx.Err(int32(C.vg_vamana_reorder_bfs(r.h, up(perm), up(invPerm), nil))); err != nil {
		return nil, nil, err
	}
	return perm, invPerm, nil
}

// Flat-segment quantization kinds of FlatBuild (flat/format.go:22-26 as the library's VG_QUANT_*).
const (
	FlatQuantNone, FlatQuantSQ8, FlatQuantPQ = int(C.VG_QUANT_NONE), int(C.VG_QUANT_SQ8), int(C.VG_QUANT_PQ)
)

// FlatBuild: flat.Writer.Flush's partitioning and quantization (flat/writer.go:99-223) on the resident rows: TrainKMeans,
// AssignPartition, the counting sort by partition (perm[new] = old; invPerm[old] = new), then the quantizer trained on and
// applied to the reordered rows.  sq / pq: the quantizer handle the kind needs (HIPScalarQuantizer.Handle() /
// HIPProductQuantizer.Handle(), the latter created as (dim, pqM, 256); pqM 0 = dim/8), nil otherwise.  The caller permutes
// what the GPU never held (ids, metadata, payloads) with perm.
func (r *Resident) FlatBuild(numPartitions, quant, pqM int, seed uint64, sq, pq unsafe.Pointer) (perm, invPerm []uint32, err error) {
	perm, invPerm = make([]uint32, r.rows), make([]uint32, r.rows)
	var pp, pi *C.uint32_t
	if r.rows > 0 {
		pp, pi = up(perm), up(invPerm)
	}
	if err := hipctx.Err(int32(C.vg_flat_build(r.h, C.int32_t(numPartitions), C.int32_t(quant), C.int32_t(pqM), 0, 0, C.uint64_t(seed),
		(*C.vg_sq8)(sq), (*C.vg_pq)(pq), pp, pi, nil))); err != nil {
		return nil, nil, err
	}
	return perm, invPerm, nil
}

// WriteFlat: the file flat.Writer.Flush writes (flat/writer.go:312-470) for the resident segment, the body's CRC-32C computed
// on the GPU.  ids in the segment's row order (nil = 0..rows-1); metadata / blockStats: the sections as Flush serialises them
// (:230-307) from the documents permuted with FlatBuild's perm, nil = the bytes of rows without documents.
func (r *Resident) WriteFlat(segmentID uint64, ids []uint64, metadata, blockStats []byte) ([]byte, error) {
	var mb, sb C.int64_t = -1, -1
	var mp, sp unsafe.Pointer
	none := []byte{0} // an empty section still travels as a non-nil pointer
	section := func(b []byte) (unsafe.Pointer, C.int64_t) {
		if len(b) == 0 {
			return unsafe.Pointer(&none[0]), 0
		}
		return unsafe.Pointer(&b[0]), C.int64_t(len(b))
	}
	if metadata != nil {
		mp, mb = section(metadata)
	}
	if blockStats != nil {
		sp, sb = section(blockStats)
	}
	size := int64(C.vg_segment_flat_image_size(r.h, mb, sb))
	if size < 0 {
		return nil, hipctx.Err(int32(C.VG_ERR_UNSUPPORTED))
	}
	if len(ids) != 0 && len(ids) != r.rows {
		return nil, fmt.Errorf("segment: WriteFlat: %d ids for %d rows", len(ids), r.rows)
	}
	var ip64 *C.uint64_t
	if len(ids) != 0 {
		ip64 = (*C.uint64_t)(unsafe.Pointer(&ids[0]))
	}
	image := make([]byte, size)
	var written C.int64_t
	if err := hipctx.Err(int32(C.vg_segment_write_flat(r.h, C.uint64_t(segmentID), ip64, mp, mb, sp, sb, unsafe.Pointer(&image[0]),
		C.int64_t(size), &written, nil))); err != nil {
		return nil, err
	}
	return image[:int(written)], nil
}

// DiskANN quantization kinds of DiskANNBuild (quantization.Type, types.go:6-14, as the library's VG_QUANT_*).
const (
	DiskANNQuantNone, DiskANNQuantPQ, DiskANNQuantRaBitQ, DiskANNQuantInt4 = int(C.VG_QUANT_NONE), int(C.VG_QUANT_PQ), int(C.VG_QUANT_RABITQ), int(C.VG_QUANT_INT4)
)

// DiskANNBuild: diskann.Writer.Write up to Flush (diskann/writer.go:217-253) on the resident rows: the quantizer trained on and
// applied to the rows in add order (pq: HIPProductQuantizer.Handle() created as (dim, pqM, 256); iq: HIPInt4Quantizer.Handle();
// nil otherwise), buildGraph, reorderBFS (perm[new] = old; invPerm[old] = new, the writer's addOrderToFinalRow).  used is the
// kind of the codes now on the segment: DiskANNQuantNone for PQ over fewer than 256 rows (trainPQ, :276-279).  The caller
// permutes what the GPU never held (ids, metadata, payloads) with perm and rebuilds its inverted index (reorder.go:138-150).
func (r *Resident) DiskANNBuild(R, L int, alpha float32, quant, pqM int, seed uint64, pq, iq unsafe.Pointer) (perm, invPerm []uint32, used int, err error) {
	perm, invPerm = make([]uint32, r.rows), make([]uint32, r.rows)
	var pp, pi *C.uint32_t
	if r.rows > 0 {
		pp, pi = up(perm), up(invPerm)
	}
	var u C.int32_t
	if err := hipctx.Err(int32(C.vg_diskann_build(r.h, C.int32_t(R), C.int32_t(L), C.float(alpha), C.int32_t(quant), C.int32_t(pqM), 0,
		C.uint64_t(seed), 8192, 32, (*C.vg_pq)(pq), (*C.vg_int4)(iq), pp, pi, &u, nil))); err != nil {
		return nil, nil, 0, err
	}
	return perm, invPerm, int(u), nil
}

// WriteDiskANN: the file diskann.Writer.Flush writes (diskann/writer.go:645-856) for the resident segment, most of the body's
// CRC-32C computed on the GPU.  searchListSize: the header's L (0 = 100); compressionType: Options.CompressionType, recorded
// only (the sections are raw, as the reference's); ids in the segment's row order (nil = 0..rows-1); metadata / metadataIndex:
// the sections as Flush serialises them (:797-833) from the documents permuted with DiskANNBuild's perm, nil = the bytes of
// rows without documents.
func (r *Resident) WriteDiskANN(segmentID uint64, searchListSize, compressionType int, ids []uint64, metadata, metadataIndex []byte) ([]byte, error) {
	var mb, xb C.int64_t = -1, -1
	var mp, xp unsafe.Pointer
	none := []byte{0} // an empty section still travels as a non-nil pointer
	section := func(b []byte) (unsafe.Pointer, C.int64_t) {
		if len(b) == 0 {
			return unsafe.Pointer(&none[0]), 0
		}
		return unsafe.Pointer(&b[0]), C.int64_t(len(b))
	}
	if metadata != nil {
		mp, mb = section(metadata)
	}
	if metadataIndex != nil {
		xp, xb = section(metadataIndex)
	}
	if len(ids) != 0 && len(ids) != r.rows {
		return nil, fmt.Errorf("segment: WriteDiskANN: %d ids for %d rows", len(ids), r.rows)
	}
	var ip64 *C.uint64_t
	if len(ids) != 0 {
		ip64 = (*C.uint64_t)(unsafe.Pointer(&ids[0]))
	}
	size := int64(C.vg_segment_diskann_image_size(r.h, mb, xb))
	if size < 0 { // the call names the refusal
		return nil, hipctx.Err(int32(C.vg_segment_write_diskann(r.h, C.uint64_t(segmentID), C.int32_t(searchListSize), C.int32_t(compressionType),
			ip64, mp, mb, xp, xb, unsafe.Pointer(&none[0]), 0, nil, nil)))
	}
	image := make([]byte, size)
	var written C.int64_t
	if err := hipctx.Err(int32(C.vg_segment_write_diskann(r.h, C.uint64_t(segmentID), C.int32_t(searchListSize), C.int32_t(compressionType),
		ip64, mp, mb, xp, xb, unsafe.Pointer(&image[0]), C.int64_t(size), &written, nil))); err != nil {
		return nil, err
	}
	return image[:int(written)], nil
}

// CRC32CDevice: hash.CRC32C (internal/hash/crc32c.go:15-17) of size bytes of device memory, computed on the GPU.
func CRC32CDevice(devicePtr unsafe.Pointer, size int64) (uint32, error) {
	p, err := hipctx.Ptr()
	if err != nil {
		return 0, err
	}
	var out C.uint32_t
	if err := hipctx.Err(int32(C.vg_crc32c_device((*C.vg_ctx)(p), unsafe.Pointer(devicePtr), C.int64_t(size), &out, nil))); err != nil {
		return 0, err
	}
	return uint32(out), nil
}

// Moves is Engine.CompactWithContext's `moves` (engine/compaction.go:159-213) by row instead of by id: OldToNew over the
// concatenated source rows (0xFFFFFFFF = deleted), NewSource / NewRow per row of the new segment.  The host keys its PK
// index update with the ids it kept.
type Moves struct {
	OldToNew  []uint32
	NewSource []int32
	NewRow    []uint32
}

// Merge: the compaction's Iterate loop (engine/compaction.go:173-218; vg_index_merge) over resident segments: the rows of
// sources[0], then sources[1], ... whose bit in deleted[s] is clear (bit i of byte i/8 = row i is deleted, the tombstone
// snapshot as bytes; deleted nil or deleted[s] empty = nothing deleted there), as a new Resident with fp32 rows only.  The
// memtable flush is the same call with one source and its HNSW tombstones.  Ids, metadata, payloads, minID / maxID and the
// manifest commit stay with the caller.
func Merge(sources []*Resident, deleted [][]byte) (*Resident, *Moves, error) {
	p, err := hipctx.Ptr()
	if err != nil {
		return nil, nil, err
	}
	ctx := (*C.vg_ctx)(p)
	if len(sources) == 0 {
		return nil, nil, hipctx.Err(int32(C.VG_ERR_INVALID_ARG))
	}
	if deleted != nil && len(deleted) != len(sources) {
		return nil, nil, fmt.Errorf("segment: Merge: %d bitmaps for %d sources", len(deleted), len(sources))
	}
	// the pointer arrays and the bitmaps travel in C memory: cgo passes no Go memory that holds Go pointers
	slot := C.size_t(unsafe.Sizeof(uintptr(0)))
	hs := (**C.vg_index)(C.calloc(C.size_t(len(sources)), slot))
	ds := (**C.uint8_t)(C.calloc(C.size_t(len(sources)), slot))
	defer C.free(unsafe.Pointer(hs))
	defer C.free(unsafe.Pointer(ds))
	hv, dv := unsafe.Slice(hs, len(sources)), unsafe.Slice(ds, len(sources))
	total := 0
	for s, src := range sources {
		if src == nil {
			return nil, nil, fmt.Errorf("segment: Merge: source %d is nil", s)
		}
		hv[s] = src.h
		total += src.rows
		if deleted == nil || len(deleted[s]) == 0 || src.rows == 0 {
			continue
		}
		if len(deleted[s]) < (src.rows+7)/8 {
			return nil, nil, fmt.Errorf("segment: Merge: deleted[%d] holds %d bytes, %d needed", s, len(deleted[s]), (src.rows+7)/8)
		}
		bits := C.CBytes(deleted[s])
		defer C.free(bits)
		dv[s] = (*C.uint8_t)(bits)
	}
	m := &Moves{OldToNew: make([]uint32, total), NewSource: make([]int32, total), NewRow: make([]uint32, total)}
	var po, pr *C.uint32_t
	var ps *C.int32_t
	if total > 0 {
		po, ps, pr = up(m.OldToNew), ip(m.NewSource), up(m.NewRow)
	}
	var out *C.vg_index
	if err := hipctx.Err(int32(C.vg_index_merge(ctx, hs, ds, C.int32_t(len(sources)), &out, po, ps, pr, nil))); err != nil {
		return nil, nil, err
	}
	live := 0
	for _, v := range m.OldToNew {
		if v != 0xFFFFFFFF {
			live++
		}
	}
	m.NewSource, m.NewRow = m.NewSource[:live], m.NewRow[:live]
	return &Resident{ctx: ctx, h: out, rows: live, dim: sources[0].dim}, m, nil
}

// CompactOptions: what Engine.CompactWithContext takes from its configuration (engine/compaction.go:104-143): the
// DiskANN threshold (0 = 10000), the flat writer's quantization (FlatQuant*, with SQ / PQ the quantizer handles FlatBuild
// takes), the DiskANN writer's R / L / Alpha (R 0 = diskann.DefaultOptions: 64, 100, 1.2) and quantization (DiskANNQuant*, with
// PQ / Int4 the handles DiskANNBuild takes).
type CompactOptions struct {
	DiskANNThreshold int
	FlatQuant        int
	DiskANNQuant     int
	PQM              int
	SQ, PQ, Int4     unsafe.Pointer
	R, L             int
	Alpha            float32
	Seed             uint64
}

// CompactionPlan: the writer the engine chooses (engine/compaction.go:86-152) for totalRows source rows, deleted ones
// included: DiskANN from the threshold up, else flat with max(1, totalRows/8192) partitions.
func CompactionPlan(totalRows, diskANNThreshold int) (diskann bool, k int) {
	if diskANNThreshold <= 0 {
		diskANNThreshold = 10000
	}
	if totalRows >= diskANNThreshold {
		return true, 0
	}
	if totalRows/8192 < 1 {
		return false, 1
	}
	return false, totalRows / 8192
}

// Compact: Merge, then the writer CompactionPlan chooses, FlatBuild or DiskANNBuild, on the result.  What the builders do
// with few rows passes through: FlatBuild leaves fewer live rows than k unpartitioned, DiskANNBuild refuses 0 rows ("no
// vectors to write").  The Moves are the FINAL positions: Merge's composed with the builder's perm / invPerm.  (The
// reference's flat NewRowID is the add order, right only for k = 1, compaction.go:205-206; these are the rows' true places.)
func Compact(sources []*Resident, deleted [][]byte, o CompactOptions) (*Resident, *Moves, bool, error) {
	total := 0
	for s, src := range sources {
		if src == nil {
			return nil, nil, false, fmt.Errorf("segment: Compact: source %d is nil", s)
		}
		total += src.rows
	}
	diskann, k := CompactionPlan(total, o.DiskANNThreshold)
	merged, m, err := Merge(sources, deleted)
	if err != nil {
		return nil, nil, false, err
	}
	var perm, inv []uint32
	if diskann {
		R, L, alpha := o.R, o.L, o.Alpha
		if R == 0 {
			R, L, alpha = 64, 100, 1.2
		}
		perm, inv, _, err = merged.DiskANNBuild(R, L, alpha, o.DiskANNQuant, o.PQM, o.Seed, o.PQ, o.Int4)
	} else {
		perm, inv, err = merged.FlatBuild(k, o.FlatQuant, o.PQM, o.Seed, o.SQ, o.PQ)
	}
	if err != nil {
		merged.Close()
		return nil, nil, false, err
	}
	f := &Moves{OldToNew: make([]uint32, len(m.OldToNew)), NewSource: make([]int32, len(perm)), NewRow: make([]uint32, len(perm))}
	for i, v := range m.OldToNew {
		f.OldToNew[i] = v
		if v != 0xFFFFFFFF {
			f.OldToNew[i] = inv[v]
		}
	}
	for j, old := range perm {
		f.NewSource[j], f.NewRow[j] = m.NewSource[old], m.NewRow[old]
	}
	return merged, f, diskann, nil
}

// VamanaGraph: (R, n*R neighbour ids with 0xFFFFFFFF = none, entry point) — what Writer.Flush writes.
func (r *Resident) VamanaGraph() (int, []uint32, uint32, error) {
	var R C.int32_t
	var entry C.uint32_t
	if err := hipctx.Err(int32(C.vg_index_get_vamana_graph(r.h, &R, &entry, nil, nil))); err != nil {
		return 0, nil, 0, err
	}
	graph := make([]uint32, r.rows*int(R))
	if len(graph) > 0 {
		if err := hipctx.Err(int32(C.vg_index_get_vamana_graph(r.h, nil, nil, up(graph), nil))); err != nil {
			return 0, nil, 0, err
		}
	}
	return int(R), graph, uint32(entry), nil
}

// ---- searches: nq row-major queries in, nq*k (RowID, Score) best-first out -----------------------------------------

func (r *Resident) out(nq, k int) ([]uint32, []float32) { return make([]uint32, nq*k), make([]float32, nq*k) }

// SearchFlat: flat.Segment.Search's fp32 branch (flat/segment.go:691-721); hnsw.BruteSearch is SearchHNSWBrute.
func (r *Resident) SearchFlat(queries []float32, nq, k int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	st := C.vg_search_flat(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchThreshold: the flat-segment leg of Engine.SearchThreshold (engine/engine.go:1485-1531): Search(q, maxResults)
// (flat/segment.go:447-721), then the rows with Score <= thresholds[q] (L2) / >= thresholds[q] (Dot, Cosine), best first.
// Query q's rows are ids/scores[q*maxResults : q*maxResults+counts[q]].  thresholds: one per query.  maxResults <= 16384;
// a segment with more than one IVF partition is refused (the reference would probe only some of them): SearchProbedThreshold.
func (r *Resident) SearchThreshold(queries []float32, nq int, thresholds []float32, maxResults int) ([]uint32, []float32, []int32, error) {
	if len(thresholds) < nq {
		return nil, nil, nil, fmt.Errorf("SearchThreshold: %d thresholds for %d queries", len(thresholds), nq)
	}
	if nq == 0 || maxResults == 0 {
		return nil, nil, make([]int32, nq), nil
	}
	ids, sc := r.out(nq, maxResults)
	counts := make([]int32, nq)
	st := C.vg_search_flat_threshold(r.h, fp(queries), C.int64_t(nq), fp(thresholds), C.int32_t(maxResults), nil, 0, up(ids), fp(sc), ip(counts), nil)
	return ids, sc, counts, hipctx.Err(int32(st))
}

// thresholdOperands: what the probed threshold searches check and allocate: one threshold per query, a mask long enough for
// its stride (nil = no filter), the result arrays.  ok == false: nothing to do (nq or maxResults is 0).
func (r *Resident) thresholdOperands(name string, nq int, thresholds []float32, maxResults int, mask []byte, maskStride int) (ids []uint32, sc []float32, counts []int32, ok bool, err error) {
	if len(thresholds) < nq {
		return nil, nil, nil, false, fmt.Errorf("%s: %d thresholds for %d queries", name, len(thresholds), nq)
	}
	counts = make([]int32, nq)
	if nq == 0 || maxResults == 0 {
		return nil, nil, counts, false, nil
	}
	if mask != nil {
		need := (r.rows + 7) / 8
		if maskStride != 0 {
			if maskStride < need {
				return nil, nil, nil, false, fmt.Errorf("%s: maskStride %d is shorter than a mask (%d bytes)", name, maskStride, need)
			}
			need += (nq - 1) * maskStride
		}
		if len(mask) < need {
			return nil, nil, nil, false, fmt.Errorf("%s: mask holds %d bytes, %d needed", name, len(mask), need)
		}
	}
	ids, sc = r.out(nq, maxResults)
	return ids, sc, counts, true, nil
}

// SearchProbedThreshold: Engine.SearchThreshold (engine/engine.go:1485-1531) over a flat segment with codes and / or IVF
// partitions (flat/segment.go:447-780): the best maxResults rows of the nprobes closest partitions (or of the whole segment)
// by the score of `scan`, then — rerank — their exact scores, then the rows with Score <= thresholds[q] (L2) / >=
// thresholds[q] (Dot, Cosine), best first.  rerank false: the threshold is compared with the scan score (the segment-level
// answer).  Query q's rows are ids/scores[q*maxResults : q*maxResults+counts[q]].  mask nil = no filter, else as for
// SearchFiltered.  maxResults <= 16384, nprobes <= 64.
func (r *Resident) SearchProbedThreshold(queries []float32, nq int, thresholds []float32, maxResults, nprobes int, scan int32, rerank bool, mask []byte, maskStride int) ([]uint32, []float32, []int32, error) {
	ids, sc, counts, ok, err := r.thresholdOperands("SearchProbedThreshold", nq, thresholds, maxResults, mask, maskStride)
	if !ok {
		return nil, nil, counts, err
	}
	var mp *C.uint8_t
	if mask != nil {
		mp = bp(mask)
	}
	rr := 0
	if rerank {
		rr = 1
	}
	st := C.vg_search_flat_probed_threshold(r.h, fp(queries), C.int64_t(nq), fp(thresholds), C.int32_t(maxResults), C.int32_t(nprobes), C.int32_t(scan), C.int32_t(rr), mp, C.int64_t(maskStride), up(ids), fp(sc), ip(counts), nil)
	return ids, sc, counts, hipctx.Err(int32(st))
}

// SearchSegmentThreshold: Engine.SearchThreshold for a segment opened from its file, by what the file holds: a flat segment
// is SearchProbedThreshold with the segment's scan, a DiskANN segment SearchVamanaThreshold with its kind (nprobes and rerank
// are unused there).
func (r *Resident) SearchSegmentThreshold(queries []float32, nq int, thresholds []float32, maxResults, nprobes int, rerank bool, mask []byte, maskStride int) ([]uint32, []float32, []int32, error) {
	ids, sc, counts, ok, err := r.thresholdOperands("SearchSegmentThreshold", nq, thresholds, maxResults, mask, maskStride)
	if !ok {
		return nil, nil, counts, err
	}
	var mp *C.uint8_t
	if mask != nil {
		mp = bp(mask)
	}
	rr := 0
	if rerank {
		rr = 1
	}
	st := C.vg_segment_search_threshold(r.seg, fp(queries), C.int64_t(nq), fp(thresholds), C.int32_t(maxResults), C.int32_t(nprobes), C.int32_t(rr), mp, C.int64_t(maskStride), up(ids), fp(sc), ip(counts), nil)
	return ids, sc, counts, hipctx.Err(int32(st))
}

// SearchPQ: the PQ branch (flat/segment.go:476-483,678-689): BuildDistanceTable + PqAdcLookup per row.
func (r *Resident) SearchPQ(queries []float32, nq, k int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	st := C.vg_search_pq_adc(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchSQ8: the SQ8 branch (flat/segment.go:517-604 L2, :659-667 Dot).
func (r *Resident) SearchSQ8(queries []float32, nq, k int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	st := C.vg_search_sq8(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// EnableSQ8Nomination: batches of SearchSQ8 are nominated by a bfloat16 MFMA GEMM over the dequantised rows (+ rows*dim*2 bytes of
// device memory) and re-scored exactly from the codes; results unchanged.
func (r *Resident) EnableSQ8Nomination(on bool) error {
	v := C.int32_t(0)
	if on {
		v = 1
	}
	return hipctx.Err(int32(C.vg_index_enable_sq8_nomination(r.h, v, nil)))
}

// EnableSQ8NominationFromCodes: the same nomination without the dequantised-row image — the queries are scaled by the inverse
// scales and the GEMM's row tiles converted from the code tiles (whole-segment, unfiltered batches above 128 queries).  Resident:
// 4 bytes a row and 4 a dimension.  The two modes are exclusive; results unchanged.
func (r *Resident) EnableSQ8NominationFromCodes(on bool) error {
	v := C.int32_t(0)
	if on {
		v = 1
	}
	return hipctx.Err(int32(C.vg_index_enable_sq8_nomination_from_codes(r.h, v, nil)))
}

// SQ8NominationInfo: mode 0 (off), 1 (the dequantised-row image) or 2 (from the codes), the device bytes the mode keeps resident,
// and the queries whose proof failed and the scan answered since the mode was enabled.
func (r *Resident) SQ8NominationInfo() (mode int, heldBytes, rescanned int64, err error) {
	var m C.int32_t
	var b, n C.int64_t
	st := C.vg_index_sq8_nomination_info(r.h, &m, &b, &n)
	return int(m), int64(b), int64(n), hipctx.Err(int32(st))
}

// EnableRaBitQNomination: batches of SearchRaBitQ above 128 queries (k <= 256, queries x rows >= 12M) are nominated by an int8 MFMA
// GEMM over the sign bits (exact Hamming distances), listed behind a conservative screen, re-scored with popcount and the
// reference's formula and proven; nothing resident; results unchanged.  An index holding a negative stored norm keeps the scan.
func (r *Resident) EnableRaBitQNomination(on bool) error {
	v := C.int32_t(0)
	if on {
		v = 1
	}
	return hipctx.Err(int32(C.vg_index_enable_rabitq_nomination(r.h, v, nil)))
}

// RaBitQNominationInfo: whether the mode is on, the device bytes it keeps resident (0), the queries whose list was incomplete and
// the scan answered since the mode was enabled, and the VG_RABITQ_NOM_CHECK hook's count of disagreeing Hamming distances.
func (r *Resident) RaBitQNominationInfo() (on bool, heldBytes, rescanned, mismatched int64, err error) {
	var m C.int32_t
	var b, n, x C.int64_t
	st := C.vg_index_rabitq_nomination_info(r.h, &m, &b, &n, &x)
	return m != 0, int64(b), int64(n), int64(x), hipctx.Err(int32(st))
}

// EnablePQNomination: batches of SearchPQ (queries x rows >= 24M, k <= 256) are nominated by a bfloat16 MFMA GEMM over the decoded
// rows (+ rows*dim*2 bytes of device memory) and re-scored from the codes against the query's distance table; results unchanged.
func (r *Resident) EnablePQNomination(on bool) error {
	v := C.int32_t(0)
	if on {
		v = 1
	}
	return hipctx.Err(int32(C.vg_index_enable_pq_nomination(r.h, v, nil)))
}

// EnablePQNominationFromCodes: the same nomination without the decoded-row image — the GEMM's row tiles are gathered from the
// decoded codebook by the codes (8 dimensions per sub-quantizer; batches above 128 queries).  Resident: 4 bytes a row and the
// codebook.  The two modes are exclusive; results unchanged.
func (r *Resident) EnablePQNominationFromCodes(on bool) error {
	v := C.int32_t(0)
	if on {
		v = 1
	}
	return hipctx.Err(int32(C.vg_index_enable_pq_nomination_from_codes(r.h, v, nil)))
}

// PQNominationInfo: mode 0 (off), 1 (the decoded-row image) or 2 (from the codes), and the device bytes the mode keeps resident.
func (r *Resident) PQNominationInfo() (mode int, heldBytes int64, err error) {
	var m C.int32_t
	var b C.int64_t
	st := C.vg_index_pq_nomination_info(r.h, &m, &b)
	return int(m), int64(b), hipctx.Err(int32(st))
}

// FlatRetried: how many queries of the fp32 flat search, since the rows were attached, the one-product bfloat16 screen left
// open and the three-product pass nominated again (a host whose neighbours lie closer than ~2^-7 relative sees it grow).
func (r *Resident) FlatRetried() (int64, error) {
	var n C.int64_t
	st := C.vg_index_flat_retried(r.h, &n, nil)
	return int64(n), hipctx.Err(int32(st))
}

// FlatAppended: the candidates the fp32 flat search's nomination appended to its queries' lists since the rows were attached,
// summed over the queries (thresholds set too high show as long lists here, too low as exhaustive queries in FlatStats).
func (r *Resident) FlatAppended() (int64, error) {
	var n C.int64_t
	st := C.vg_index_flat_appended(r.h, &n, nil)
	return int64(n), hipctx.Err(int32(st))
}

// SearchRaBitQ: exhaustive scan of the RaBitQ codes (rq.Distance per row).
func (r *Resident) SearchRaBitQ(queries []float32, nq, k int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	st := C.vg_search_rabitq(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchInt4: exhaustive scan of the INT4 codes of a DiskANN segment (iq.L2Distance per row, the walk's own score), the k best by
// (Score, RowID), scores ascending under every metric; k <= 512.  mask nil: every row takes part; else bit i of byte i/8 =
// filter.Matches(i), len(mask) == ceil(rows/8) for one mask (maskStride 0) or (nq-1)*maskStride + ceil(rows/8) for one per query.
func (r *Resident) SearchInt4(queries []float32, nq, k int, mask []byte, maskStride int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	var pm *C.uint8_t
	if mask != nil {
		need := (r.rows + 7) / 8
		if maskStride != 0 {
			if maskStride < need {
				return nil, nil, fmt.Errorf("SearchInt4: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
			}
			need += (nq - 1) * maskStride
		}
		if len(mask) < need || len(mask) == 0 {
			return nil, nil, fmt.Errorf("SearchInt4: mask holds %d bytes, %d needed", len(mask), need)
		}
		pm = bp(mask)
	}
	st := C.vg_search_int4(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), pm, C.int64_t(maskStride), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchProbed: a partitioned flat segment, only the nprobes closest partitions (flat/segment.go:727-749).
func (r *Resident) SearchProbed(queries []float32, nq, k, nprobes int, scan int32) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	st := C.vg_search_flat_probed(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(nprobes), C.int32_t(scan), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchSegmentFiltered: Segment.Search with a filter for a segment opened from its file (flat or DiskANN, by what it holds).
func (r *Resident) SearchSegmentFiltered(queries []float32, nq, k, nprobes int, mask []byte, maskStride int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	need := (r.rows + 7) / 8
	if maskStride != 0 {
		if maskStride < need {
			return nil, nil, fmt.Errorf("SearchSegmentFiltered: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
		}
		need += (nq - 1) * maskStride
	}
	if len(mask) < need {
		return nil, nil, fmt.Errorf("SearchSegmentFiltered: mask holds %d bytes, %d needed", len(mask), need)
	}
	st := C.vg_segment_search_filtered(r.seg, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(nprobes), bp(mask), C.int64_t(maskStride), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchFiltered: Segment.Search with `filter segment.Filter` set (flat/segment.go:631-635, :559-561): rows whose mask bit
// is clear are skipped.  mask: bit i of byte i/8 = filter.Matches(i), len(mask) == ceil(rows/8) for one mask (maskStride 0)
// or (nq-1)*maskStride + ceil(rows/8) for one per query.
func (r *Resident) SearchFiltered(queries []float32, nq, k, nprobes int, scan int32, mask []byte, maskStride int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	need := (r.rows + 7) / 8
	if maskStride != 0 {
		if maskStride < need {
			return nil, nil, fmt.Errorf("SearchFiltered: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
		}
		need += (nq - 1) * maskStride
	}
	if len(mask) < need {
		return nil, nil, fmt.Errorf("SearchFiltered: mask holds %d bytes, %d needed", len(mask), need)
	}
	st := C.vg_search_flat_filtered(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(nprobes), C.int32_t(scan), bp(mask), C.int64_t(maskStride), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// Search: the whole of Segment.Search for a segment opened from its file: scan type / beam search by what the
// file holds.
func (r *Resident) Search(queries []float32, nq, k, nprobes int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	st := C.vg_segment_search(r.seg, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(nprobes), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchHNSW: hnsw.KNNSearch (hnsw.go:1650-1755).  stats may be nil; otherwise len(stats) >= nq.
func (r *Resident) SearchHNSW(queries []float32, nq, k, ef int, stats []Stats) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	var sp *C.vg_search_stats
	if len(stats) >= nq && nq > 0 {
		sp = (*C.vg_search_stats)(unsafe.Pointer(&stats[0]))
	}
	st := C.vg_search_hnsw(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(ef), up(ids), fp(sc), sp, nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchHNSWPQ: the graph walked on PQ codes (distFunc = pq.ComputeAsymmetricDistance, diskann/segment.go:536-557);
// follow with Rerank (engine/search.go:914-965).
func (r *Resident) SearchHNSWPQ(queries []float32, nq, k, ef int, stats []Stats) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	var sp *C.vg_search_stats
	if len(stats) >= nq && nq > 0 {
		sp = (*C.vg_search_stats)(unsafe.Pointer(&stats[0]))
	}
	st := C.vg_search_hnsw_pq(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(ef), up(ids), fp(sc), sp, nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchHNSWFiltered: searchExecute with a filter and a selectivity hint above 0.3 — searchLayerWithPostFilter
// (hnsw.go:1159-1218).  mask: bit i of byte i/8 = row i passes (filter.Matches and not tombstoned), len(mask) ==
// ceil(n/8) for one mask (maskStride 0) or nq*maskStride; ef is what determineEF returned.  A selectivity at or below
// 0.3 (or unknown, < 0) is routed by the library to the predicate-aware walk, as searchExecute does (hnsw.go:1086-1157):
// the same as calling SearchHNSWPredicate.
func (r *Resident) SearchHNSWFiltered(queries []float32, nq, k, ef int, mask []byte, maskStride int, selectivity float64, stats []Stats) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	need := (r.rows + 7) / 8
	if maskStride != 0 {
		if maskStride < need {
			return nil, nil, fmt.Errorf("SearchHNSWFiltered: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
		}
		need += (nq - 1) * maskStride
	}
	if len(mask) < need {
		return nil, nil, fmt.Errorf("SearchHNSWFiltered: mask holds %d bytes, %d needed", len(mask), need)
	}
	var sp *C.vg_search_stats
	if len(stats) >= nq && nq > 0 {
		sp = (*C.vg_search_stats)(unsafe.Pointer(&stats[0]))
	}
	st := C.vg_search_hnsw_filtered(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(ef), bp(mask), C.int64_t(maskStride), C.double(selectivity), up(ids), fp(sc), sp, nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchHNSWPredicate: searchExecute with a filter whose selectivity hint is at or below 0.3, or unknown —
// searchLayerPredicateAware (hnsw.go:1406-1558).  mask as for SearchHNSWFiltered (filter.Matches only); deleted: the
// tombstone bitmap (ceil(n/8) bytes) or nil.  stats[i].ShortCircuits = ExpansionsSkipped.
func (r *Resident) SearchHNSWPredicate(queries []float32, nq, k, ef int, mask []byte, maskStride int, deleted []byte, stats []Stats) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	need := (r.rows + 7) / 8
	if len(deleted) > 0 && len(deleted) < need {
		return nil, nil, fmt.Errorf("SearchHNSWPredicate: deleted holds %d bytes, %d needed", len(deleted), need)
	}
	if maskStride != 0 {
		if maskStride < need {
			return nil, nil, fmt.Errorf("SearchHNSWPredicate: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
		}
		need += (nq - 1) * maskStride
	}
	if len(mask) < need {
		return nil, nil, fmt.Errorf("SearchHNSWPredicate: mask holds %d bytes, %d needed", len(mask), need)
	}
	var sp *C.vg_search_stats
	if len(stats) >= nq && nq > 0 {
		sp = (*C.vg_search_stats)(unsafe.Pointer(&stats[0]))
	}
	var dp *C.uint8_t
	if len(deleted) > 0 {
		dp = bp(deleted)
	}
	st := C.vg_search_hnsw_predicate(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(ef), bp(mask), C.int64_t(maskStride), dp, up(ids), fp(sc), sp, nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SetHNSWTombstones: g.tombstones (hnsw.go:95) as a bitmap, ceil(rows/8) bytes, nil = none: deleted nodes are walked
// through but never returned by the HNSW searches (hnsw.go:1381-1390).
func (r *Resident) SetHNSWTombstones(deleted []byte) error {
	if len(deleted) == 0 {
		return hipctx.Err(int32(C.vg_index_set_hnsw_tombstones(r.h, nil, nil)))
	}
	if need := (r.rows + 7) / 8; len(deleted) < need {
		return fmt.Errorf("SetHNSWTombstones: bitmap holds %d bytes, %d needed", len(deleted), need)
	}
	return hipctx.Err(int32(C.vg_index_set_hnsw_tombstones(r.h, bp(deleted), nil)))
}

// SetHNSWEdgeDistances: the layer-0 lists' cached Neighbor.Dist (node.go:62-80), rows*m0 values slot for slot with the uploaded
// lists; nil = recompute them from the fp32 rows.
func (r *Resident) SetHNSWEdgeDistances(l0Dist []float32) error {
	var p *C.float
	if len(l0Dist) > 0 {
		p = fp(l0Dist)
	}
	return hipctx.Err(int32(C.vg_index_set_hnsw_edge_distances(r.h, p, nil)))
}

// BruteMode selects which of the HNSW index's exhaustive paths SearchHNSWBrute replays.
type BruteMode int32

const (
	BruteScan   BruteMode = 0 // hnsw.BruteSearch + scanSegment (hnsw.go:2021-2101): PopItem + PushItem
	BruteBitmap BruteMode = 1 // searchBitmap (hnsw.go:2240-2263): TryPushBounded(k)
)

// SearchHNSWBrute: BruteSearch / searchBitmap over the rows whose bit is set in mask (bit i of byte i/8; nil =
// every row; len(mask) == ceil(n/8) for one mask, nq*maskStride for one per query), in ascending id through the
// reference's PriorityQueue: ids AND their order among equal distances are the reference's.  Distances are the
// index's (L2, -dot, 0.5*L2), best first.
func (r *Resident) SearchHNSWBrute(queries []float32, nq, k int, mode BruteMode, mask []byte, maskStride int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	var mp *C.uint8_t
	if len(mask) > 0 {
		// the library reads ceil(rows/8) bytes per mask, query q's at q*maskStride: a shorter slice would be read past its end
		need := (r.rows + 7) / 8
		if maskStride != 0 {
			if maskStride < need {
				return nil, nil, fmt.Errorf("SearchHNSWBrute: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
			}
			need += (nq - 1) * maskStride
		}
		if len(mask) < need {
			return nil, nil, fmt.Errorf("SearchHNSWBrute: mask holds %d bytes, %d needed", len(mask), need)
		}
		mp = (*C.uint8_t)(unsafe.Pointer(&mask[0]))
	}
	st := C.vg_search_hnsw_brute(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(mode), mp, C.int64_t(maskStride), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchVamana: diskann searchInternal (diskann/segment.go:503-706) with the given node scorer.
func (r *Resident) SearchVamana(queries []float32, nq, k, kind int, stats []Stats) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	var sp *C.vg_search_stats
	if len(stats) >= nq && nq > 0 {
		sp = (*C.vg_search_stats)(unsafe.Pointer(&stats[0]))
	}
	st := C.vg_search_vamana(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(kind), up(ids), fp(sc), sp, nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchVamanaFiltered: searchInternal with `filter` set (diskann/segment.go:616-627): a row whose mask bit is clear is walked
// through but never enters the result heap.  mask as for SearchFiltered.
func (r *Resident) SearchVamanaFiltered(queries []float32, nq, k, kind int, mask []byte, maskStride int, stats []Stats) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	need := (r.rows + 7) / 8
	if maskStride != 0 {
		if maskStride < need {
			return nil, nil, fmt.Errorf("SearchVamanaFiltered: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
		}
		need += (nq - 1) * maskStride
	}
	if len(mask) < need {
		return nil, nil, fmt.Errorf("SearchVamanaFiltered: mask holds %d bytes, %d needed", len(mask), need)
	}
	var sp *C.vg_search_stats
	if len(stats) >= nq && nq > 0 {
		sp = (*C.vg_search_stats)(unsafe.Pointer(&stats[0]))
	}
	st := C.vg_search_vamana_filtered(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(kind), bp(mask), C.int64_t(maskStride), up(ids), fp(sc), sp, nil)
	return ids, sc, hipctx.Err(int32(st))
}

// SearchVamanaThreshold: the DiskANN leg of Engine.SearchThreshold (engine/engine.go:1485-1531): SearchVamanaFiltered(q,
// maxResults), then the rows with Score <= thresholds[q] (L2) / >= thresholds[q] (Dot, Cosine) in walk order.  Query q's rows
// are ids/scores[q*maxResults : q*maxResults+counts[q]].  mask nil = no filter, else as for SearchVamanaFiltered.
// maxResults <= 16384.
func (r *Resident) SearchVamanaThreshold(queries []float32, nq int, thresholds []float32, maxResults, kind int, mask []byte, maskStride int, stats []Stats) ([]uint32, []float32, []int32, error) {
	if len(thresholds) < nq {
		return nil, nil, nil, fmt.Errorf("SearchVamanaThreshold: %d thresholds for %d queries", len(thresholds), nq)
	}
	if nq == 0 || maxResults == 0 {
		return nil, nil, make([]int32, nq), nil
	}
	if mask != nil {
		need := (r.rows + 7) / 8
		if maskStride != 0 {
			if maskStride < need {
				return nil, nil, nil, fmt.Errorf("SearchVamanaThreshold: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
			}
			need += (nq - 1) * maskStride
		}
		if len(mask) < need {
			return nil, nil, nil, fmt.Errorf("SearchVamanaThreshold: mask holds %d bytes, %d needed", len(mask), need)
		}
	}
	ids, sc := r.out(nq, maxResults)
	counts := make([]int32, nq)
	var sp *C.vg_search_stats
	if len(stats) >= nq {
		sp = (*C.vg_search_stats)(unsafe.Pointer(&stats[0]))
	}
	var mp *C.uint8_t
	if mask != nil {
		mp = bp(mask)
	}
	st := C.vg_search_vamana_threshold(r.h, fp(queries), C.int64_t(nq), fp(thresholds), C.int32_t(maxResults), C.int32_t(kind), mp, C.int64_t(maskStride), up(ids), fp(sc), ip(counts), sp, nil)
	return ids, sc, counts, hipctx.Err(int32(st))
}

// SearchVamanaFresh: FreshVamana.Search, and with a mask SearchWithFilter (diskann/fresh_vamana.go:272-364), over the resident
// Vamana graph (vg_search_vamana_fresh).  L = the index's search list size (0 = 100); deleted as for InsertVamana; mask /
// maskStride as for SearchVamanaThreshold.  Query q's rows are ids[q*k : q*k+counts[q]].
func (r *Resident) SearchVamanaFresh(queries []float32, nq, k, L int, deleted, mask []byte, maskStride int) ([]uint32, []float32, []int32, error) {
	if nq == 0 || k == 0 {
		return nil, nil, make([]int32, nq), nil
	}
	need := (r.rows + 7) / 8
	var dp, mp *C.uint8_t
	if deleted != nil && need > 0 {
		if len(deleted) < need {
			return nil, nil, nil, fmt.Errorf("SearchVamanaFresh: deleted holds %d bytes, %d needed", len(deleted), need)
		}
		dp = bp(deleted)
	}
	if mask != nil {
		if maskStride != 0 {
			if maskStride < need {
				return nil, nil, nil, fmt.Errorf("SearchVamanaFresh: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
			}
			need += (nq - 1) * maskStride
		}
		if len(mask) < need || len(mask) == 0 {
			return nil, nil, nil, fmt.Errorf("SearchVamanaFresh: mask holds %d bytes, %d needed", len(mask), need)
		}
		mp = bp(mask)
	}
	ids, sc := r.out(nq, k)
	counts := make([]int32, nq)
	st := C.vg_search_vamana_fresh(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), C.int32_t(L), dp, mp, C.int64_t(maskStride), up(ids), fp(sc), ip(counts), nil)
	return ids, sc, counts, hipctx.Err(int32(st))
}

// Rerank: Segment.Rerank + top-k (flat/segment.go:754-780, engine/search.go:914-965): nc candidate rows per query.
func (r *Resident) Rerank(queries []float32, nq int, candidates []uint32, nc, k int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	st := C.vg_rerank(r.h, fp(queries), C.int64_t(nq), up(candidates), C.int32_t(nc), C.int32_t(k), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}

// MergeTopK: the engine's fan-in over segments (engine/search.go:904-908) for `lists` resident segments' results:
// ties by (score, RowID + idOffsets[list]).
func MergeTopK(idsIn []uint32, scoresIn []float32, lists, nq, k int, metric distance.Metric, idOffsets []uint32) ([]uint32, []float32, error) {
	p, err := hipctx.Ptr()
	if err != nil {
		return nil, nil, err
	}
	ids, sc := make([]uint32, nq*k), make([]float32, nq*k)
	var off *C.uint32_t
	if len(idOffsets) > 0 {
		off = up(idOffsets)
	}
	st := C.vg_merge_topk((*C.vg_ctx)(p), up(idsIn), fp(scoresIn), C.int32_t(lists), C.int64_t(nq), C.int32_t(k), C.int32_t(metric), off,
		up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}
