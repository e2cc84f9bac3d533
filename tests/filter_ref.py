"""The numpy restatement of the filter semantics vg_filter_evaluate implements (include/vecgo_hip.h, "Metadata filters on
the device"): presence, the six compares of compareFloat64, eq / in on dictionary codes, AND over a filter set, an empty set
matches every row, a field without a column matches nothing, deleted rows cleared, tail bits of the last byte zero.  The
tests compare the library against this, bit for bit; tests/test_filter_ref_cpu.py pins this against cases from the
reference's own tests."""
import numpy as np

INVALID_ID = 0xFFFFFFFF
OPS = ("eq", "ne", "lt", "lte", "gt", "gte", "in")


class RefColumns:
    """field -> ("f64", values float64[rows], present bool[rows]) or ("codes", codes uint32[rows])"""

    def __init__(self, rows):
        self.rows = rows
        self.cols = {}

    def set_f64(self, field, values, present=None):
        values = np.asarray(values, np.float64)
        assert values.shape == (self.rows,)
        present = np.ones(self.rows, bool) if present is None else np.asarray(present, bool)
        self.cols[field] = ("f64", values, present)

    def set_codes(self, field, codes):
        codes = np.asarray(codes, np.uint32)
        assert codes.shape == (self.rows,)
        self.cols[field] = ("codes", codes)

    def drop(self, field):
        self.cols.pop(field, None)


def _op_name(op):
    return op.lower() if isinstance(op, str) else OPS[int(op)]


def match_filter(cols: RefColumns, field, op, operand):
    """bool[rows]: the rows one filter matches"""
    op = _op_name(op)
    col = cols.cols.get(field)
    if col is None:                       # a field the segment does not have matches nothing
        return np.zeros(cols.rows, bool)
    if col[0] == "f64":
        _, v, present = col
        c = np.float64(operand)
        with np.errstate(invalid="ignore"):
            hit = {"eq": v == c, "ne": v != c, "lt": v < c, "lte": v <= c, "gt": v > c, "gte": v >= c}[op]   # IEEE: compareFloat64
        return hit & present              # a row without the field never matches, `ne` included
    _, codes = col
    has = codes != INVALID_ID
    if op == "eq":
        return has & (codes == np.uint32(operand))
    if op == "in":
        return has & np.isin(codes, np.asarray(operand, np.uint32).reshape(-1))   # an empty set matches nothing
    raise ValueError(f"{op} on a code column")


def match_set(cols: RefColumns, filters, deleted=None):
    """bool[rows]: the AND of the filters (an empty set: every row), less the deleted rows"""
    m = np.ones(cols.rows, bool)
    for field, op, operand in filters:
        m &= match_filter(cols, field, op, operand)
    if deleted is not None:
        m &= ~np.asarray(deleted, bool)
    return m


def pack(bits):
    """bool[..., rows] -> uint8[..., ceil(rows / 8)]: bit i of byte i / 8, tail bits of the last byte zero"""
    bits = np.asarray(bits, bool)
    if bits.shape[-1] == 0:
        return np.zeros(bits.shape[:-1] + (0,), np.uint8)
    return np.packbits(bits, axis=-1, bitorder="little")


def evaluate(cols: RefColumns, filter_sets, deleted=None):
    """(masks uint8[nq, ceil(rows / 8)], counts int64[nq]) of a batch of filter sets"""
    rows = [match_set(cols, fs, deleted) for fs in filter_sets]
    bits = np.stack(rows) if rows else np.zeros((0, cols.rows), bool)
    return pack(bits), bits.sum(axis=1).astype(np.int64)
