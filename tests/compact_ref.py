"""Engine.CompactWithContext (internal/engine/compaction.go:86-218) up to the writer, restated in numpy: the Iterate loop
with its tombstone check, the choice of writer, and the composition of the loop's move maps with a builder's permutation.
What the GPU merge (vg_index_merge) and vecgo_amd.compact are compared with; tests/test_merge_cpu.py checks this helper
against a literal double loop."""
import numpy as np

INVALID = 0xFFFFFFFF


def unpack(bits, n):
    """bool[n] from a tombstone bitmap: bit i of byte i/8, bits at or above n ignored; None = nothing deleted; a bool
    array passes through"""
    if bits is None:
        return np.zeros(n, bool)
    b = np.asarray(bits)
    if b.dtype == np.bool_:
        assert b.size == n
        return b.copy()
    return np.unpackbits(np.ascontiguousarray(b, np.uint8), bitorder="little")[:n].astype(bool)


def merge(sources, deleted=None):
    """compaction.go:173-218: for every segment in order, for every row in order (flat/segment.go:1028-1073), skip the row if
    the segment's tombstones contain it (:179), else add it; count is its new row (:207-212).
    sources: list of [n_s, dim] fp32; deleted: None or one bitmap / bool array / None per source.
    Returns (rows [live, dim], old_to_new [sum n_s] uint32 with INVALID for deleted rows, new_source [live] int32,
    new_row [live] uint32)."""
    dim = sources[0].shape[1]
    dead = [unpack(None if deleted is None else deleted[s], len(x)) for s, x in enumerate(sources)]
    live = ~np.concatenate(dead) if dead else np.zeros(0, bool)
    all_rows = np.concatenate([np.asarray(x, np.float32).reshape(-1, dim) for x in sources])
    src_of = np.concatenate([np.full(len(x), s, np.int32) for s, x in enumerate(sources)])
    row_of = np.concatenate([np.arange(len(x), dtype=np.uint32) for x in sources])
    old_to_new = np.full(live.size, INVALID, np.uint32)
    old_to_new[live] = np.arange(int(live.sum()), dtype=np.uint32)
    return np.ascontiguousarray(all_rows[live]), old_to_new, src_of[live], row_of[live]


def plan(total_rows, diskann_threshold=0):
    """compaction.go:86-152: totalRows sums RowCount() of the segments, deleted rows included (:87-90); the DiskANN
    threshold is 10000 unless the configured one is positive (:104-107); totalRows >= threshold takes DiskANN (:113), else
    flat with k = int(totalRows / 8192), at least 1 (:137-140)."""
    threshold = 10000
    if diskann_threshold > 0:
        threshold = diskann_threshold
    if total_rows >= threshold:
        return "diskann", 0
    k = total_rows // 8192
    if k < 1:
        k = 1
    return "flat", k


def compose(old_to_new, new_source, new_row, perm, inv_perm):
    """the loop's maps through a builder's order (perm[final] = merged row, inv_perm[merged row] = final): where every
    source row finally sits and where every final row came from"""
    final = old_to_new.copy()
    live = old_to_new != INVALID
    final[live] = np.asarray(inv_perm, np.uint32)[old_to_new[live]]
    return final, new_source[perm], new_row[perm]
