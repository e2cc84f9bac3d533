//go:build hip && cgo

// A lexical.Index whose Search runs on the device: the resident BM25 index (vg_bm25) behind the interface of
// lexical/bm25.MemoryIndex, and the Reciprocal Rank Fusion of Engine.HybridSearch (internal/engine/engine.go:1560-1602) for
// a batch.  The seams are WithLexicalIndex (the engine takes any lexical.Index) and the fusion loop of HybridSearch.  What is
// text stays here: the tokeniser, the term dictionary, math.Log for the idf and the doc -> primary key map.  Writes follow
// the index onto the device: Add and Delete queue into a pending batch, and the next Search flushes it with ONE
// vg_bm25_update (the first flush into a vg_bm25_create_empty index), which rewrites the resident image on the device;
// nothing is sorted or uploaded again.  For that the dictionary is APPEND-ONLY: a term keeps its id for good, a term whose
// list has emptied keeps an empty range on the device and is skipped in a query (the reference deletes the list,
// bm25.go:259-261).  The document frequencies come from the host's own lists.  upload() — the whole image from host arrays,
// lists sorted by doc, as vg_bm25_create wants them — remains as the recovery path after a failed update.
package lexical

/*
#cgo CFLAGS: -I${SRCDIR}/../../third_party/vecgo_hip/include
#cgo LDFLAGS: -L${SRCDIR}/../../third_party/vecgo_hip -lvecgo_hip
#include "vecgo_hip.h"
*/
import "C"

import (
	"context"
	"math"
	"sort"
	"strings"
	"sync"
	"unicode"
	"unsafe"

	"github.com/hupe1980/vecgo/internal/hipctx"
	"github.com/hupe1980/vecgo/model"
)

type hipPosting struct {
	doc, tf uint32
}

// HipIndex implements Index.
type HipIndex struct {
	mu  sync.Mutex
	ctx *C.vg_ctx
	h   *C.vg_bm25

	pkToDoc    map[model.ID]uint32
	docToPK    []model.ID
	freeDocs   []uint32
	docLengths []uint32
	docTerms   [][]string
	docTf      [][]uint32 // the counts of docTerms, entry for entry
	inverted   map[string][]hipPosting
	dict       map[string]uint32 // term -> id: append-only, ids are never reassigned
	resident   []bool            // per doc: does the device image hold a document in this slot?
	touched    map[uint32]bool   // the pending batch: doc -> resident[doc] when the batch first touched it

	totalLength int64
	docCount    int
	dirty       bool // the device image cannot be trusted (a failed update): the next Search rebuilds it with upload()
}

var _ Index = (*HipIndex)(nil)

func u32p(p []uint32) *C.uint32_t {
	if len(p) == 0 {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&p[0]))
}

func i32p(p []int32) *C.int32_t {
	if len(p) == 0 {
		return nil
	}
	return (*C.int32_t)(unsafe.Pointer(&p[0]))
}

func i64p(p []int64) *C.int64_t {
	if len(p) == 0 {
		return nil
	}
	return (*C.int64_t)(unsafe.Pointer(&p[0]))
}

func f64p(p []float64) *C.double {
	if len(p) == 0 {
		return nil
	}
	return (*C.double)(unsafe.Pointer(&p[0]))
}

func f32p(p []float32) *C.float {
	if len(p) == 0 {
		return nil
	}
	return (*C.float)(unsafe.Pointer(&p[0]))
}

// NewHipIndex creates an empty index on device 0.
func NewHipIndex() (*HipIndex, error) {
	p, err := hipctx.Ptr()
	if err != nil {
		return nil, err
	}
	return &HipIndex{ctx: (*C.vg_ctx)(p), pkToDoc: map[model.ID]uint32{}, inverted: map[string][]hipPosting{}, dict: map[string]uint32{},
		touched: map[uint32]bool{}}, nil
}

// tokens: whitespace-separated, lower-cased; pure ASCII text splits at every byte up to ' ' and lowers A-Z only, other
// text splits at unicode.IsSpace and lowers rune by rune (the reference tokeniser's two paths).
func tokens(text string) []string {
	ascii := true
	for i := 0; i < len(text); i++ {
		if text[i] >= 0x80 {
			ascii = false
			break
		}
	}
	if ascii {
		f := strings.FieldsFunc(text, func(r rune) bool { return r <= ' ' })
		for i, t := range f {
			f[i] = strings.Map(func(r rune) rune {
				if r >= 'A' && r <= 'Z' {
					return r + ('a' - 'A')
				}
				return r
			}, t)
		}
		return f
	}
	f := strings.FieldsFunc(text, unicode.IsSpace)
	for i, t := range f {
		f[i] = strings.Map(unicode.ToLower, t)
	}
	return f
}

// Add indexes a document, replacing an earlier one under the same id.
func (x *HipIndex) Add(id model.ID, text string) error {
	x.mu.Lock()
	defer x.mu.Unlock()
	if _, ok := x.pkToDoc[id]; ok {
		x.remove(id)
	}
	var doc uint32
	if n := len(x.freeDocs); n > 0 {
		doc = x.freeDocs[n-1]
		x.freeDocs = x.freeDocs[:n-1]
		x.docToPK[doc] = id
	} else {
		doc = uint32(len(x.docToPK))
		x.docToPK = append(x.docToPK, id)
		x.docLengths = append(x.docLengths, 0)
		x.docTerms = append(x.docTerms, nil)
		x.docTf = append(x.docTf, nil)
		x.resident = append(x.resident, false)
	}
	x.touch(doc)
	x.pkToDoc[id] = doc
	tf := map[string]uint32{}
	length := 0
	for _, t := range tokens(text) {
		length++
		tf[t]++
	}
	x.docLengths[doc] = uint32(length)
	x.totalLength += int64(length)
	x.docCount++
	terms := make([]string, 0, len(tf))
	counts := make([]uint32, 0, len(tf))
	for t, c := range tf {
		terms = append(terms, t)
		counts = append(counts, c)
		x.inverted[t] = append(x.inverted[t], hipPosting{doc: doc, tf: c})
		if _, ok := x.dict[t]; !ok {
			x.dict[t] = uint32(len(x.dict))
		}
	}
	x.docTerms[doc] = terms
	x.docTf[doc] = counts
	return nil
}

// touch notes that the pending batch changes doc, and whether the device image held a document there before it.
func (x *HipIndex) touch(doc uint32) {
	if _, ok := x.touched[doc]; !ok {
		x.touched[doc] = x.resident[doc]
	}
}

// Delete removes a document; its doc slot keeps length 0 and is reused by a later Add.
func (x *HipIndex) Delete(id model.ID) error {
	x.mu.Lock()
	defer x.mu.Unlock()
	x.remove(id)
	return nil
}

func (x *HipIndex) remove(id model.ID) {
	doc, ok := x.pkToDoc[id]
	if !ok {
		return
	}
	x.touch(doc)
	for _, t := range x.docTerms[doc] {
		list := x.inverted[t]
		for i := range list {
			if list[i].doc == doc {
				list = append(list[:i], list[i+1:]...)
				break
			}
		}
		if len(list) == 0 {
			delete(x.inverted, t)
		} else {
			x.inverted[t] = list
		}
	}
	x.totalLength -= int64(x.docLengths[doc])
	x.docCount--
	x.docLengths[doc] = 0
	x.docToPK[doc] = 0
	x.docTerms[doc] = nil
	x.docTf[doc] = nil
	delete(x.pkToDoc, id)
	x.freeDocs = append(x.freeDocs, doc)
}

func (x *HipIndex) drop() {
	if x.h != nil {
		C.vg_bm25_destroy(x.h)
		x.h = nil
	}
}

// flush applies the pending batch with one vg_bm25_update: the docs the device holds and the batch touched are deleted,
// the touched docs that hold a document now are added (a doc in both lists is a replace).  Term ids are the dictionary's.
func (x *HipIndex) flush() error {
	if x.h == nil {
		if st := C.vg_bm25_create_empty(x.ctx, C.int32_t(0), &x.h); st != C.VG_OK {
			return hipctx.Err(int32(st))
		}
	}
	var del, docs, lens, terms, tfs []uint32
	off := make([]int64, 1, len(x.touched)+1)
	for doc, had := range x.touched {
		if had {
			del = append(del, doc)
		}
		if x.docTerms[doc] == nil {
			continue
		}
		docs = append(docs, doc)
		lens = append(lens, x.docLengths[doc])
		for i, t := range x.docTerms[doc] {
			terms = append(terms, x.dict[t])
			tfs = append(tfs, x.docTf[doc][i])
		}
		off = append(off, int64(len(terms)))
	}
	st := C.vg_bm25_update(x.h, u32p(del), C.int64_t(len(del)), u32p(docs), u32p(lens), nil, C.int64_t(len(docs)), i64p(off), u32p(terms), u32p(tfs),
		C.int64_t(len(x.docLengths)), C.int64_t(len(x.dict)), C.int64_t(x.totalLength), C.int64_t(x.docCount), nil)
	if st != C.VG_OK {
		x.dirty = true // the image is as it was before the call, the batch is not in it: rebuild
		return hipctx.Err(int32(st))
	}
	for _, doc := range del {
		x.resident[doc] = false
	}
	for _, doc := range docs {
		x.resident[doc] = true
	}
	x.touched = map[uint32]bool{}
	return nil
}

// upload replaces the device image from the host's lists (the recovery path after a failed update): CSR postings under the
// dictionary's ids — a term without a list is an empty range — with every list sorted by doc.
func (x *HipIndex) upload() error {
	x.drop()
	names := make([]string, len(x.dict))
	for t, id := range x.dict {
		names[id] = t
	}
	off := make([]int64, 1, len(names)+1)
	var docs, tfs []uint32
	for _, t := range names {
		list := append([]hipPosting(nil), x.inverted[t]...)
		sort.Slice(list, func(a, b int) bool { return list[a].doc < list[b].doc })
		for _, p := range list {
			docs = append(docs, p.doc)
			tfs = append(tfs, p.tf)
		}
		off = append(off, int64(len(docs)))
	}
	st := C.vg_bm25_create(x.ctx, C.int64_t(len(x.docLengths)), C.int64_t(len(names)), i64p(off), u32p(docs), u32p(tfs), u32p(x.docLengths),
		C.int64_t(x.totalLength), C.int64_t(x.docCount), nil, &x.h)
	if st != C.VG_OK {
		return hipctx.Err(int32(st))
	}
	for doc := range x.resident {
		x.resident[doc] = x.docTerms[doc] != nil
	}
	x.touched = map[uint32]bool{}
	x.dirty = false
	return nil
}

// queryArrays: the term ids of the texts' tokens that have a posting list — a term whose list has emptied is skipped, as the
// reference has deleted it — with the reference's idf (math.Log(1 + (N - n + 0.5) / (n + 0.5))) per entry, n from the
// host's own list.
func (x *HipIndex) queryArrays(texts []string) ([]int32, []uint32, []float64) {
	off := make([]int32, 1, len(texts)+1)
	var terms []uint32
	var idf []float64
	n := float64(x.docCount)
	for _, text := range texts {
		for _, t := range tokens(text) {
			list := x.inverted[t]
			if len(list) == 0 {
				continue
			}
			df := float64(len(list))
			terms = append(terms, x.dict[t])
			idf = append(idf, math.Log(1+(n-df+0.5)/(df+0.5)))
		}
		off = append(off, int32(len(terms)))
	}
	return off, terms, idf
}

// SearchBatch answers every text with its best k docs: doc ids (VG_INVALID_ID behind a short list), float32 scores and the
// number of hits per query.
func (x *HipIndex) SearchBatch(texts []string, k int) ([]uint32, []float32, []int32, error) {
	x.mu.Lock()
	defer x.mu.Unlock()
	return x.searchLocked(texts, k)
}

func (x *HipIndex) searchLocked(texts []string, k int) ([]uint32, []float32, []int32, error) {
	nq := len(texts)
	ids := make([]uint32, nq*k)
	scores := make([]float32, nq*k)
	counts := make([]int32, nq)
	if x.docCount == 0 || nq == 0 || k == 0 {
		for i := range ids {
			ids[i] = 0xFFFFFFFF
			scores[i] = float32(math.Inf(-1))
		}
		return ids, scores, counts, nil
	}
	if x.dirty {
		if err := x.upload(); err != nil {
			return nil, nil, nil, err
		}
	} else if x.h == nil || len(x.touched) > 0 {
		if err := x.flush(); err != nil {
			return nil, nil, nil, err
		}
	}
	off, terms, idf := x.queryArrays(texts)
	st := C.vg_bm25_search(x.h, i32p(off), u32p(terms), f64p(idf), C.int64_t(nq), C.int32_t(k), u32p(ids), f32p(scores), i32p(counts), nil)
	if st != C.VG_OK {
		return nil, nil, nil, hipctx.Err(int32(st))
	}
	return ids, scores, counts, nil
}

// Search implements Index: one query, candidates under their primary keys, best first.
func (x *HipIndex) Search(ctx context.Context, text string, k int) ([]model.Candidate, error) {
	if err := ctx.Err(); err != nil {
		return nil, err
	}
	x.mu.Lock()
	defer x.mu.Unlock()
	ids, scores, counts, err := x.searchLocked([]string{text}, k)
	if err != nil {
		return nil, err
	}
	if counts[0] == 0 {
		return nil, nil
	}
	out := make([]model.Candidate, counts[0])
	for i := range out {
		out[i] = model.Candidate{ID: x.docToPK[ids[i]], Score: scores[i]}
	}
	return out, nil
}

// Replayed: the queries since the index was made (updates keep the count) whose tied scores went through the reference's heap on the device.
func (x *HipIndex) Replayed() (int64, error) {
	x.mu.Lock()
	defer x.mu.Unlock()
	if x.h == nil {
		return 0, nil
	}
	var n C.int64_t
	if st := C.vg_bm25_replayed(x.h, &n, nil); st != C.VG_OK {
		return 0, hipctx.Err(int32(st))
	}
	return int64(n), nil
}

// ResidentBytes: what the index holds on the device, the spare image of the updates included.
func (x *HipIndex) ResidentBytes() (int64, error) {
	x.mu.Lock()
	defer x.mu.Unlock()
	if x.h == nil {
		return 0, nil
	}
	var docs, terms, postings, bytes C.int64_t
	if st := C.vg_bm25_stats(x.h, &docs, &terms, &postings, &bytes); st != C.VG_OK {
		return 0, hipctx.Err(int32(st))
	}
	return int64(bytes), nil
}

// Export copies the resident image out (what persists an index the host never assembled): the term offsets, the postings
// and the doc lengths, under the dictionary's term ids.  Pending writes are flushed first.
func (x *HipIndex) Export() ([]int64, []uint32, []uint32, []uint32, error) {
	x.mu.Lock()
	defer x.mu.Unlock()
	if x.dirty {
		if err := x.upload(); err != nil {
			return nil, nil, nil, nil, err
		}
	} else if x.h == nil || len(x.touched) > 0 {
		if err := x.flush(); err != nil {
			return nil, nil, nil, nil, err
		}
	}
	var nDocs, nTerms, nPost, bytes C.int64_t
	if st := C.vg_bm25_stats(x.h, &nDocs, &nTerms, &nPost, &bytes); st != C.VG_OK {
		return nil, nil, nil, nil, hipctx.Err(int32(st))
	}
	off := make([]int64, int(nTerms)+1)
	docs := make([]uint32, int(nPost))
	tfs := make([]uint32, int(nPost))
	lens := make([]uint32, int(nDocs))
	if st := C.vg_bm25_export(x.h, i64p(off), u32p(docs), u32p(tfs), u32p(lens), nil, nil); st != C.VG_OK {
		return nil, nil, nil, nil, hipctx.Err(int32(st))
	}
	return off, docs, tfs, lens, nil
}

// Close implements Index.
func (x *HipIndex) Close() error {
	x.mu.Lock()
	defer x.mu.Unlock()
	x.drop()
	return nil
}

// FuseRRF is the fusion of Engine.HybridSearch for a batch: list A (the vector results) sets 1 / float32(rrfK + rank + 1)
// per id, list B (the lexical results) adds it; the best k per query by score, ties by ascending id.  aIDs / bIDs hold
// aStride / bStride slots per query of which aCounts[q] / bCounts[q] are used.
func FuseRRF(aIDs []uint32, aCounts []int32, aStride int, bIDs []uint32, bCounts []int32, bStride int, rrfK, k int) ([]uint32, []float32, []int32, error) {
	p, err := hipctx.Ptr()
	if err != nil {
		return nil, nil, nil, err
	}
	nq := len(aCounts)
	if nq == 0 {
		nq = len(bCounts)
	}
	ids := make([]uint32, nq*k)
	scores := make([]float32, nq*k)
	counts := make([]int32, nq)
	st := C.vg_rrf_fuse((*C.vg_ctx)(p), C.int64_t(nq), u32p(aIDs), i32p(aCounts), C.int64_t(aStride), u32p(bIDs), i32p(bCounts), C.int64_t(bStride),
		C.int32_t(rrfK), C.int32_t(k), u32p(ids), f32p(scores), i32p(counts), nil)
	if st != C.VG_OK {
		return nil, nil, nil, hipctx.Err(int32(st))
	}
	return ids, scores, counts, nil
}
