//go:build hip && cgo

// Metadata filters on the device: the resident metadata columns of a segment (numeric fields as float64 with a presence
// bitmap, categorical fields as dictionary codes) and UnifiedIndex.EvaluateFilter (internal/metadata/unified.go:279-416)
// for a whole query batch, written straight into device masks that the Resident filtered searches read.  The seams are
// Engine.evaluateSegmentFilterResult (engine/search.go:1176) and UnifiedIndex.EvaluateFilter; the value -> code
// dictionary, Set / Delete bookkeeping and uploading a column again after writes stay on the Go side.
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

	"github.com/hupe1980/vecgo/internal/hipctx"
)

// metadata.Operator as vg_filter_clause.op.
const (
	FilterEQ = int32(C.VG_FILTER_EQ)
	FilterNE = int32(C.VG_FILTER_NE)
	FilterLT = int32(C.VG_FILTER_LT)
	FilterLE = int32(C.VG_FILTER_LTE)
	FilterGT = int32(C.VG_FILTER_GT)
	FilterGE = int32(C.VG_FILTER_GTE)
	FilterIN = int32(C.VG_FILTER_IN)
)

// simd.AndWords / AndNotWords / OrWords / XorWords (internal/simd/bitmap.go:26-48).
const (
	MaskAnd    = int32(C.VG_MASK_AND)
	MaskAndNot = int32(C.VG_MASK_ANDNOT)
	MaskOr     = int32(C.VG_MASK_OR)
	MaskXor    = int32(C.VG_MASK_XOR)
)

// NoCode is the code of a row without a value, and of a value the dictionary does not hold: no row matches it.
const NoCode = uint32(0xFFFFFFFF)

// Filter is one metadata.Filter against a resident column.  Value is read for a float64 column, Code (FilterEQ) and
// Codes (FilterIN) for a code column.
type Filter struct {
	Field int
	Op    int32
	Value float64
	Code  uint32
	Codes []uint32
}

// Columns are the resident metadata columns of one segment (vg_columns).
type Columns struct {
	ctx  *C.vg_ctx
	h    *C.vg_columns
	rows int
}

func dp(p []float64) *C.double { return (*C.double)(unsafe.Pointer(&p[0])) }

func lp(p []int64) *C.int64_t { return (*C.int64_t)(unsafe.Pointer(&p[0])) }

// NewColumns creates the empty column set of a segment of `rows` rows.
func NewColumns(rows int) (*Columns, error) {
	p, err := hipctx.Ptr()
	if err != nil {
		return nil, err
	}
	c := &Columns{ctx: (*C.vg_ctx)(p), rows: rows}
	if st := C.vg_columns_create(c.ctx, C.int64_t(rows), &c.h); st != C.VG_OK {
		return nil, hipctx.Err(int32(st))
	}
	return c, nil
}

// Close frees the device memory.
func (c *Columns) Close() {
	if c.h != nil {
		C.vg_columns_destroy(c.h)
		c.h = nil
	}
}

// SetFloat64 uploads a numeric field (ints as float64(I64), numeric_index.go:1072-1076): one value per row; present:
// bit i of byte i/8 = row i has a value, nil = every row.  It replaces whatever the field held.
func (c *Columns) SetFloat64(field int, values []float64, present []byte) error {
	if len(values) != c.rows {
		return fmt.Errorf("segment: SetFloat64: %d values for %d rows", len(values), c.rows)
	}
	if present != nil && len(present) < (c.rows+7)/8 {
		return fmt.Errorf("segment: SetFloat64: present holds %d bytes, %d needed", len(present), (c.rows+7)/8)
	}
	var vp *C.double
	var pp *C.uint8_t
	if c.rows > 0 {
		vp = dp(values)
		if present != nil {
			pp = bp(present)
		}
	}
	return hipctx.Err(int32(C.vg_columns_set_f64(c.h, C.int32_t(field), vp, pp, nil)))
}

// SetCodes uploads a categorical field as dictionary codes: one per row, NoCode = the row has no value.
func (c *Columns) SetCodes(field int, codes []uint32) error {
	if len(codes) != c.rows {
		return fmt.Errorf("segment: SetCodes: %d codes for %d rows", len(codes), c.rows)
	}
	var cp *C.uint32_t
	if c.rows > 0 {
		cp = up(codes)
	}
	return hipctx.Err(int32(C.vg_columns_set_codes(c.h, C.int32_t(field), cp, nil)))
}

// Drop leaves the field without a column: a filter on it then matches nothing.
func (c *Columns) Drop(field int) error {
	return hipctx.Err(int32(C.vg_columns_drop(c.h, C.int32_t(field))))
}

// DeviceMasks are the row masks of a query batch in device memory: mask q starts Stride bytes after mask q-1.
// Counts[q] is the number of rows query q's filter set matches (the selectivity numerator).
type DeviceMasks struct {
	ctx    *C.vg_ctx
	p      *C.uint8_t
	rows   int
	NQ     int
	Stride int
	Counts []int64
}

// Bytes is the device memory as a slice, to be handed with Stride to SearchFiltered, SearchSegmentFiltered,
// SearchHNSWFiltered, SearchHNSWPredicate and the other Resident calls that take mask / maskStride: the library reads
// the masks where they lie.  The slice must never be read or written on the host.
func (m *DeviceMasks) Bytes() []byte {
	if m.p == nil {
		return nil
	}
	return unsafe.Slice((*byte)(unsafe.Pointer(m.p)), m.NQ*m.Stride)
}

// Combine joins a mask made on the host (`contains`, string ranges: what the device does not evaluate) into every
// query's mask: mask[q] = mask[q] op hostMask (vg_mask_combine).
func (m *DeviceMasks) Combine(op int32, hostMask []byte) error {
	if len(hostMask) < (m.rows+7)/8 {
		return fmt.Errorf("segment: Combine: mask holds %d bytes, %d needed", len(hostMask), (m.rows+7)/8)
	}
	if m.p == nil {
		return nil
	}
	return hipctx.Err(int32(C.vg_mask_combine(m.ctx, C.int32_t(op), m.p, C.int64_t(m.Stride), bp(hostMask), 0, C.int64_t(m.NQ), C.int64_t(m.rows), nil)))
}

// Popcount counts the masks again (after Combine): Counts is refreshed and returned (vg_mask_popcount).
func (m *DeviceMasks) Popcount() ([]int64, error) {
	if m.p == nil {
		return m.Counts, nil
	}
	err := hipctx.Err(int32(C.vg_mask_popcount(m.ctx, m.p, C.int64_t(m.Stride), C.int64_t(m.NQ), C.int64_t(m.rows), lp(m.Counts), nil)))
	return m.Counts, err
}

// Free releases the device memory.
func (m *DeviceMasks) Free() {
	if m.p != nil {
		C.vg_mask_free(m.ctx, m.p)
		m.p = nil
	}
}

// EvaluateFilters: UnifiedIndex.EvaluateFilter for a batch (vg_filter_evaluate): sets[q] is query q's filter set (the AND
// of its filters; empty = every row), deleted the segment's tombstones (bit i of byte i/8 = row i is deleted; nil =
// none), cleared from every mask.  Only the predicates cross to the device.
func (r *Resident) EvaluateFilters(cols *Columns, sets [][]Filter, deleted []byte) (*DeviceMasks, error) {
	if cols == nil || cols.rows != r.rows {
		return nil, fmt.Errorf("segment: EvaluateFilters: the columns are not this segment's (%d rows)", r.rows)
	}
	nq := len(sets)
	off := make([]int32, nq+1)
	var cl []C.vg_filter_clause
	var codes []uint32
	for q, fs := range sets {
		for _, f := range fs {
			c := C.vg_filter_clause{field: C.int32_t(f.Field), op: C.int32_t(f.Op), value: C.double(f.Value), code: C.uint32_t(f.Code)}
			if f.Op == FilterIN {
				c.set_begin, c.set_count = C.int32_t(len(codes)), C.int32_t(len(f.Codes))
				codes = append(codes, f.Codes...)
			}
			cl = append(cl, c)
		}
		off[q+1] = int32(len(cl))
	}
	need := (r.rows + 7) / 8
	stride := (need + 7) &^ 7
	m := &DeviceMasks{ctx: r.ctx, rows: r.rows, NQ: nq, Stride: stride, Counts: make([]int64, nq)}
	if nq == 0 || r.rows == 0 {
		return m, nil
	}
	if deleted != nil && len(deleted) < need {
		return nil, fmt.Errorf("segment: EvaluateFilters: deleted holds %d bytes, %d needed", len(deleted), need)
	}
	if st := C.vg_mask_alloc(r.ctx, C.int64_t(nq*stride), &m.p); st != C.VG_OK {
		return nil, hipctx.Err(int32(st))
	}
	var cp *C.vg_filter_clause
	if len(cl) > 0 {
		cp = (*C.vg_filter_clause)(unsafe.Pointer(&cl[0]))
	}
	var sp *C.uint32_t
	if len(codes) > 0 {
		sp = up(codes)
	}
	var del *C.uint8_t
	if deleted != nil {
		del = bp(deleted)
	}
	st := C.vg_filter_evaluate(cols.h, cp, ip(off), C.int64_t(nq), sp, C.int64_t(len(codes)), del, m.p, C.int64_t(stride), lp(m.Counts), nil)
	if st != C.VG_OK {
		m.Free()
		return nil, hipctx.Err(int32(st))
	}
	return m, nil
}

// MaskRows: FilterResult.ToArrayInto for the batch (vg_mask_to_rows; engine/search.go:617-627): per query the ids of the
// rows its mask keeps, ascending, at most outStride of them, the rest of its outStride slots NoCode (VG_INVALID_ID) — the
// block feeds Rerank as it is.  The masks' Counts are refreshed: all set bits, also past outStride.
func (m *DeviceMasks) MaskRows(outStride int) ([]uint32, error) {
	if outStride < 0 {
		return nil, fmt.Errorf("segment: MaskRows: outStride %d is negative", outStride)
	}
	rows := make([]uint32, m.NQ*outStride)
	if m.p == nil || m.NQ == 0 {
		return rows, nil
	}
	var rp *C.uint32_t
	if len(rows) > 0 {
		rp = up(rows)
	}
	err := hipctx.Err(int32(C.vg_mask_to_rows(m.ctx, m.p, C.int64_t(m.Stride), C.int64_t(m.NQ), C.int64_t(m.rows), rp, C.int64_t(outStride), lp(m.Counts), nil)))
	return rows, err
}

// SearchPrefilter: the engine's bitmap strategy over this segment (vg_search_flat_prefilter; engine/search.go:602-736):
// only the rows a query's mask keeps are fetched and scored (distance.SquaredL2 / Dot), the best k by (Score, RowID) kept.
// The host picks it, as Engine.SearchIter does (selectivityCutoff / adaptiveThreshold, :572-586), from the masks' Counts.
// mask / maskStride as SearchFiltered's (DeviceMasks.Bytes() and Stride, or host bytes; maskStride 0 = one mask for the
// batch); IVF partitions are ignored.  k <= 16384.
func (r *Resident) SearchPrefilter(queries []float32, nq, k int, mask []byte, maskStride int) ([]uint32, []float32, error) {
	ids, sc := r.out(nq, k)
	need := (r.rows + 7) / 8
	if maskStride != 0 {
		if maskStride < need {
			return nil, nil, fmt.Errorf("SearchPrefilter: maskStride %d is shorter than a mask (%d bytes)", maskStride, need)
		}
		need += (nq - 1) * maskStride
	}
	if mask == nil || len(mask) < need {
		return nil, nil, fmt.Errorf("SearchPrefilter: mask holds %d bytes, %d needed", len(mask), need)
	}
	if nq == 0 || k == 0 {
		return ids, sc, nil
	}
	st := C.vg_search_flat_prefilter(r.h, fp(queries), C.int64_t(nq), C.int32_t(k), bp(mask), C.int64_t(maskStride), up(ids), fp(sc), nil)
	return ids, sc, hipctx.Err(int32(st))
}
