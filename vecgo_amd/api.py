"""Python mirror of the reference interfaces over the C ABI (tests + bench driver).

Arrays may be numpy (host) or torch CUDA tensors (HBM); the library detects which.
"""
from __future__ import annotations

import ctypes as C
import enum

import numpy as np

from . import _lib
from ._lib import VecgoHipError, check

try:  # torch is plumbing only: device buffers and streams
    import torch
except Exception:  # pragma: no cover
    torch = None


class Metric(enum.IntEnum):
    """distance.Metric (distance/distance.go:66-73)."""
    L2 = 0
    COSINE = 1
    DOT = 2
    HAMMING = 3


def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def _ptr(x, dtype, count=None):
    """(keepalive, void*) of a contiguous numpy array or torch tensor of `dtype`."""
    if x is None:
        return None, None
    if _is_torch(x):
        tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.int8: torch.int8,
               np.uint32: torch.int32, np.int32: torch.int32, np.uint64: torch.int64,
               np.int64: torch.int64}[dtype]
        if x.dtype != tdt:
            raise TypeError(f"expected torch dtype {tdt}, got {x.dtype}")
        if not x.is_contiguous():
            x = x.contiguous()
        if count is not None and x.numel() < count:
            raise ValueError(f"buffer has {x.numel()} elements, need {count}")
        return x, C.c_void_p(x.data_ptr())
    a = np.ascontiguousarray(x, dtype=dtype)
    if count is not None and a.size < count:
        raise ValueError(f"buffer has {a.size} elements, need {count}")
    return a, C.c_void_p(a.ctypes.data)


def _stream_ptr(stream):
    if stream is None:
        # Device tensors handed to the library are produced on torch's current stream; run on
        # it by default so that producer and consumer are ordered.  (The C ABI's own default,
        # NULL = the context's private stream, is for host-buffer callers such as cgo.)
        if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
            return _handle(torch.cuda.current_stream().cuda_stream)
        return None
    if torch is not None and isinstance(stream, torch.cuda.Stream):
        return _handle(stream.cuda_stream)
    return _handle(int(stream))


def _handle(h: int):
    # torch's default stream is HIP's legacy default stream, handle 0; the C ABI reserves NULL
    # for "the context's own stream", so the legacy stream travels as VG_STREAM_LEGACY (= 1)
    return C.c_void_p(h if h != 0 else 1)


class Context:
    """One per (process, GPU)."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.vg_ctx_create(C.c_int32(device), C.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vg_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self, stream=None):
        check(self._lib.vg_ctx_synchronize(self._h, _stream_ptr(stream)))

    def profile_enable(self, on: bool = True):
        check(self._lib.vg_profile_enable(self._h, C.c_int32(1 if on else 0)))

    def profile_read(self, kernel: str):
        """(launches, total_ms) of `kernel` since the last read (HIP events on the launch stream)."""
        n = C.c_int64(); ms = C.c_double()
        check(self._lib.vg_profile_read(self._h, kernel.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def device_info(self):
        arch = C.create_string_buffer(64)
        cus = C.c_int32()
        hbm = C.c_int64()
        check(self._lib.vg_ctx_device_info(self._h, arch, 64, C.byref(cus), C.byref(hbm)))
        return {"arch": arch.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}


def squared_l2_batch(ctx: Context, query, targets, dim: int, out=None, stream=None):
    """simd.SquaredL2Batch (internal/simd/kernels.go:66-68)."""
    return _batch(ctx, ctx._lib.vg_squared_l2_batch, query, targets, dim, out, stream)


def dot_batch(ctx: Context, query, targets, dim: int, out=None, stream=None):
    """simd.DotBatch (internal/simd/kernels.go:61-63)."""
    return _batch(ctx, ctx._lib.vg_dot_batch, query, targets, dim, out, stream)


def _batch(ctx, fn, query, targets, dim, out, stream):
    n = (targets.numel() if _is_torch(targets) else np.asarray(targets).size) // dim if dim > 0 else 0
    q, pq_ = _ptr(query, np.float32)
    t, pt = _ptr(targets, np.float32)
    if out is None:
        out = _empty_like(targets, (n,), np.float32)
    o, po = _ptr(out, np.float32, n)
    check(fn(ctx._h, pq_, pt, C.c_int64(dim), C.c_int64(n), po, _stream_ptr(stream)))
    return out


def merge_topk(ctx: Context, ids_in, scores_in, k: int, metric=0, id_offsets=None, out=None,
               stream=None):
    """engine fan-in (engine/search.go:904-908): ids_in/scores_in are [lists, nq, k]."""
    shape = tuple(ids_in.shape)
    lists, nq = shape[0], shape[1]
    assert shape[2] == k
    i, pi = _ptr(ids_in, np.uint32)
    s, ps = _ptr(scores_in, np.float32)
    o, po = _ptr(id_offsets, np.uint32, lists) if id_offsets is not None else (None, None)
    if out is None:
        out = (_empty_like(ids_in, (nq, k), np.uint32), _empty_like(ids_in, (nq, k), np.float32))
    oi, poi = _ptr(out[0], np.uint32, nq * k)
    os_, pos = _ptr(out[1], np.float32, nq * k)
    check(ctx._lib.vg_merge_topk(ctx._h, pi, ps, C.c_int32(lists), C.c_int64(nq), C.c_int32(k),
                                 C.c_int32(int(metric)), po, poi, pos, _stream_ptr(stream)))
    return out


class OptimizedProductQuantizer:
    """quantization.OptimizedProductQuantizer (opq.go): block-diagonal rotation + ProductQuantizer."""

    def __init__(self, ctx: Context, dimension: int, num_subvectors: int, num_centroids: int = 256, num_iterations: int = 2):
        self._lib = ctx._lib
        self._lib.vg_opq_pq.restype = C.c_void_p
        self.ctx, self.dimension, self.num_subvectors, self.num_centroids = ctx, dimension, num_subvectors, num_centroids
        h = C.c_void_p()
        check(self._lib.vg_opq_create(ctx._h, C.c_int32(dimension), C.c_int32(num_subvectors), C.c_int32(num_centroids),
                                      C.c_int32(num_iterations), C.byref(h)))
        self._h = h
        self.pq = ProductQuantizer._borrowed(ctx, C.c_void_p(self._lib.vg_opq_pq(h)), dimension, num_subvectors, num_centroids, self)
        b, nb = C.c_int32(), C.c_int32()
        check(self._lib.vg_opq_get_rotations(h, C.byref(b), C.byref(nb), None))
        self.block, self.nblocks = b.value, nb.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vg_opq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def is_trained(self) -> bool:
        return bool(self._lib.vg_opq_is_trained(self._h))

    def rotations(self):
        r = np.empty((self.nblocks, self.block, self.block), np.float32)
        check(self._lib.vg_opq_get_rotations(self._h, None, None, C.c_void_p(r.ctypes.data)))
        return r

    def set_rotations(self, rotations):
        r = np.ascontiguousarray(rotations, np.float32)
        assert r.size == self.nblocks * self.block * self.block
        check(self._lib.vg_opq_set_rotations(self._h, C.c_void_p(r.ctypes.data)))

    def train(self, vectors, pq_iters: int = 20, seed: int = 1, stream=None):
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        check(self._lib.vg_opq_train(self._h, pv, C.c_int64(n), C.c_int32(pq_iters), C.c_uint64(seed), _stream_ptr(stream)))

    def rotate(self, vectors, out=None, stream=None):
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        if out is None:
            out = _empty_like(vectors, (n, self.dimension), np.float32)
        o, po = _ptr(out, np.float32, n * self.dimension)
        check(self._lib.vg_opq_rotate(self._h, pv, C.c_int64(n), po, _stream_ptr(stream)))
        return out

    def encode(self, vectors, out=None, stream=None):
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        if out is None:
            out = _empty_like(vectors, (n, self.num_subvectors), np.uint8)
        o, po = _ptr(out, np.uint8, n * self.num_subvectors)
        check(self._lib.vg_opq_encode(self._h, pv, C.c_int64(n), po, _stream_ptr(stream)))
        return out

    def decode(self, codes, out=None, stream=None):
        c, pc = _ptr(codes, np.uint8)
        n = (c.numel() if _is_torch(c) else c.size) // self.num_subvectors
        if out is None:
            out = _empty_like(codes, (n, self.dimension), np.float32)
        o, po = _ptr(out, np.float32, n * self.dimension)
        check(self._lib.vg_opq_decode(self._h, pc, C.c_int64(n), po, _stream_ptr(stream)))
        return out

    def asymmetric_distance(self, query, codes, out=None, stream=None):
        c, pc = _ptr(codes, np.uint8)
        n = (c.numel() if _is_torch(c) else c.size) // self.num_subvectors
        q, pq_ = _ptr(query, np.float32, self.dimension)
        if out is None:
            out = _empty_like(codes, (n,), np.float32)
        o, po = _ptr(out, np.float32, n)
        check(self._lib.vg_opq_asymmetric_distance_batch(self._h, pq_, pc, C.c_int64(n), po, _stream_ptr(stream)))
        return out


class BinaryQuantizer:
    """quantization.BinaryQuantizer (binary.go:23-262): 1 bit per dimension against a threshold."""

    def __init__(self, ctx: Context, dimension: int):
        self._lib = ctx._lib
        self._lib.vg_binary_code_bytes.restype = C.c_int64
        self.ctx, self.dimension = ctx, dimension
        self.threshold, self.trained = np.float32(0.0), False

    def with_threshold(self, threshold: float):
        self.threshold, self.trained = np.float32(threshold), True
        return self

    @property
    def words(self) -> int:
        return (self.dimension + 63) // 64

    def bytes_total(self) -> int:            # BytesTotal (binary.go:198-200)
        return (self.dimension + 7) // 8

    def train(self, vectors, stream=None):
        n = _rows(vectors, self.dimension)
        if n == 0:
            raise ValueError("no vectors provided for training")
        v, pv = _ptr(vectors, np.float32)
        th = np.zeros(1, np.float32)
        check(self._lib.vg_binary_train(self.ctx._h, C.c_int32(self.dimension), pv, C.c_int64(n),
                                        C.c_void_p(th.ctypes.data), _stream_ptr(stream)))
        self.threshold, self.trained = th[0], True

    def encode(self, vectors, out=None, stream=None):
        """[n, dim] float32 -> [n, words*8] uint8 (the uint64 words of EncodeUint64Into, little endian)."""
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        if out is None:
            out = _empty_like(vectors, (n, self.words * 8), np.uint8)
        o, po = _ptr(out, np.uint8, n * self.words * 8)
        check(self._lib.vg_binary_encode(self.ctx._h, C.c_int32(self.dimension), C.c_float(float(self.threshold)), pv,
                                         C.c_int64(n), po, _stream_ptr(stream)))
        return out

    def decode(self, codes, out=None, stream=None):
        c, pc = _ptr(codes, np.uint8)
        total = c.numel() if _is_torch(c) else c.size
        cb = c.shape[-1] if len(c.shape) > 1 else total
        n = total // max(cb, 1)
        if out is None:
            out = _empty_like(codes, (n, self.dimension), np.float32)
        o, po = _ptr(out, np.float32, n * self.dimension)
        check(self._lib.vg_binary_decode(self.ctx._h, C.c_int32(self.dimension), C.c_float(float(self.threshold)), pc,
                                         C.c_int64(n), C.c_int32(cb), po, _stream_ptr(stream)))
        return out

    def compute_hamming_distance(self, query, codes, out=None, stream=None):
        """ComputeHammingDistance (binary.go:158-171) of one float query against [n, words*8] codes."""
        c, pc = _ptr(codes, np.uint8)
        n = (c.numel() if _is_torch(c) else c.size) // (self.words * 8)
        q, pq_ = _ptr(query, np.float32, self.dimension)
        if out is None:
            out = _empty_like(codes, (n,), np.int32)
        o, po = _ptr(out, np.int32, n)
        check(self._lib.vg_binary_hamming_batch(self.ctx._h, C.c_int32(self.dimension), C.c_float(float(self.threshold)),
                                                pq_, pc, C.c_int64(n), po, _stream_ptr(stream)))
        return out


def normalize_l2(ctx: Context, vectors, dim: int, stream=None):
    """distance.NormalizeL2InPlace over the rows of `vectors` (in place); returns ok[n] uint8."""
    n = _rows(vectors, dim)
    v, pv = _ptr(vectors, np.float32)
    ok = _empty_like(vectors, (n,), np.uint8)
    o, po = _ptr(ok, np.uint8, n)
    check(ctx._lib.vg_normalize_l2(ctx._h, pv, C.c_int64(n), C.c_int32(dim), po, _stream_ptr(stream)))
    return ok


class debug_hook:
    """with vecgo_amd.api.debug_hook("VG_FLAT_FORCE_EXACT"): ... — a test hook switched on for the block
    (vg_debug_set_hook)."""

    def __init__(self, *names):
        self.names = names

    def __enter__(self):
        lib = _lib.load()
        for n in self.names:
            check(lib.vg_debug_set_hook(n.encode(), 1))
        return self

    def __exit__(self, *exc):
        lib = _lib.load()
        for n in self.names:
            lib.vg_debug_set_hook(n.encode(), 0)
        return False


class Comm:
    """vg_comm: the exchange step of a row-sharded search through the C ABI (direct ncclAllGather on the
    caller's stream + merge).  Rank 0 makes the id (Comm.unique_id()), the host distributes the bytes."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        lib = _lib.load()
        buf = (C.c_uint8 * Comm.ID_BYTES)()
        check(lib.vg_comm_unique_id(buf))
        return bytes(buf)

    @staticmethod
    def probe() -> str:
        """Load RCCL (not a collective) and return the file it came from; raises when it cannot be loaded.  Every
        rank calls this and the ranks agree on the outcome BEFORE any of them enters Comm(), which is a collective."""
        lib = _lib.load()
        buf = C.create_string_buffer(1024)
        check(lib.vg_comm_probe(buf, C.c_int32(1024)))
        return buf.value.decode()

    def describe(self) -> dict:
        """What RCCL says about this communicator (ncclCommCount / UserRank / CuDevice) and which librccl is in use."""
        n, r, d, reused = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        buf = C.create_string_buffer(1024)
        check(self._lib.vg_comm_describe(self._h, C.byref(n), C.byref(r), C.byref(d), C.byref(reused), buf, C.c_int32(1024)))
        return {"rccl_ranks": n.value, "rccl_rank": r.value, "rccl_device": d.value,
                "reused_mapped_rccl": bool(reused.value), "rccl_path": buf.value.decode()}

    def __init__(self, ctx: Context, world: int, rank: int, unique_id: bytes):
        self._lib = ctx._lib
        self.ctx, self.world, self.rank = ctx, world, rank
        h = C.c_void_p()
        buf = (C.c_uint8 * Comm.ID_BYTES).from_buffer_copy(unique_id)
        check(self._lib.vg_comm_create(ctx._h, C.c_int32(world), C.c_int32(rank), buf, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vg_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def all_gather_topk(self, local_ids, local_scores, k: int, metric=0, id_offsets=None, out=None, stream=None):
        """local_ids/local_scores [nq, k] (device) -> merged global (ids, scores) [nq, k]."""
        nq = local_ids.shape[0]
        i, pi = _ptr(local_ids, np.uint32, nq * k)
        s_, ps = _ptr(local_scores, np.float32, nq * k)
        o, po = _ptr(id_offsets, np.uint32, self.world) if id_offsets is not None else (None, None)
        if out is None:
            out = (_empty_like(local_ids, (nq, k), np.uint32), _empty_like(local_ids, (nq, k), np.float32))
        oi, poi = _ptr(out[0], np.uint32, nq * k)
        os_, pos = _ptr(out[1], np.float32, nq * k)
        check(self._lib.vg_comm_all_gather_topk(self._h, pi, ps, C.c_int64(nq), C.c_int32(k), C.c_int32(int(metric)),
                                                po, poi, pos, _stream_ptr(stream)))
        return out

    def all_gather_bytes(self, send, recv, stream=None):
        """send: uint8 device tensor of this rank; recv: uint8 device tensor, world times as long."""
        a, pa = _ptr(send, np.uint8)
        b, pb = _ptr(recv, np.uint8, a.numel() * self.world)
        check(self._lib.vg_comm_all_gather(self._h, pa, pb, C.c_int64(a.numel()), _stream_ptr(stream)))
        return recv


def heap_replay(ctx: Context, is_max: bool, ops, unsigned_keys: bool = False, cap: int = 4096, stream=None):
    """vg_debug_heap_replay: ops int32[n, 4] = {op (VG_HEAP_*), node, float32 bits, arg}; returns (out int32[n, 3]
    {flag, node, bits}, nodes uint32[len], dists float32[len]) — the device heap of csrc/vg_heap.hpp after the script."""
    ops = np.ascontiguousarray(ops, np.int32).reshape(-1, 4)
    out = np.zeros((ops.shape[0], 3), np.int32)
    items = np.zeros(max(cap, 1), np.uint64)
    flen = np.zeros(1, np.int32)
    check(ctx._lib.vg_debug_heap_replay(ctx._h, C.c_int32(int(bool(is_max))), C.c_int32(int(bool(unsigned_keys))),
                                        C.c_void_p(ops.ctypes.data), C.c_int32(ops.shape[0]), C.c_void_p(out.ctypes.data),
                                        C.c_void_p(flen.ctypes.data), C.c_void_p(items.ctypes.data), C.c_int32(cap),
                                        _stream_ptr(stream)))
    items = items[:int(flen[0])]
    return out, (items & 0xFFFFFFFF).astype(np.uint32), (items >> 32).astype(np.uint32).view(np.float32)


def merge_topk_packed(ctx: Context, packed, lists: int, nq: int, k: int, metric=0, id_offsets=None, out=None, stream=None):
    """vg_merge_topk_packed: packed is a device int32/uint32 tensor [lists, 2, nq, k]."""
    p_, pp = _ptr(packed, np.uint32, lists * 2 * nq * k)
    o, po = _ptr(id_offsets, np.uint32, lists) if id_offsets is not None else (None, None)
    if out is None:
        out = (_empty_like(packed, (nq, k), np.uint32), _empty_like(packed, (nq, k), np.float32))
    oi, poi = _ptr(out[0], np.uint32, nq * k)
    os_, pos = _ptr(out[1], np.float32, nq * k)
    check(ctx._lib.vg_merge_topk_packed(ctx._h, pp, C.c_int32(lists), C.c_int64(nq), C.c_int32(k), C.c_int32(int(metric)),
                                        po, poi, pos, _stream_ptr(stream)))
    return out


def squared_l2_bounded_batch(ctx: Context, query, targets, dim: int, bounds, stream=None):
    """simd.SquaredL2Bounded (kernels.go:173), one query vs n targets: (dist[n], exceeded[n])."""
    n = (targets.numel() if _is_torch(targets) else np.asarray(targets).size) // dim if dim > 0 else 0
    q, pq_ = _ptr(query, np.float32)
    t, pt = _ptr(targets, np.float32)
    b = np.atleast_1d(np.asarray(bounds, np.float32)) if not _is_torch(bounds) else bounds
    b_, pb = _ptr(b, np.float32)
    nb = b_.numel() if _is_torch(b_) else b_.size
    dist = _empty_like(targets, (n,), np.float32)
    exc = _empty_like(targets, (n,), np.int32)
    d, pd = _ptr(dist, np.float32, n)
    e, pe = _ptr(exc, np.int32, n)
    check(ctx._lib.vg_squared_l2_bounded_batch(ctx._h, pq_, pt, C.c_int64(dim), C.c_int64(n), pb,
                                               C.c_int64(nb), pd, pe, _stream_ptr(stream)))
    return dist, exc


def pq_adc_lookup_batch(ctx: Context, table, codes, m: int, stream=None):
    """simd.PqAdcLookup (kernels.go:56), one table vs n codes."""
    n = (codes.numel() if _is_torch(codes) else np.asarray(codes).size) // m if m > 0 else 0
    t, pt = _ptr(table, np.float32, m * 256)
    c, pc = _ptr(codes, np.uint8)
    out = _empty_like(codes, (n,), np.float32)
    o, po = _ptr(out, np.float32, n)
    check(ctx._lib.vg_pq_adc_lookup_batch(ctx._h, pt, pc, C.c_int64(m), C.c_int64(n), po, _stream_ptr(stream)))
    return out


def kmeans_train(ctx: Context, vectors, dim: int, k: int, metric=0, max_iter: int = 10, seed: int = 1, stream=None):
    """kmeans.TrainKMeans (kmeans.go:16-138): returns [k, dim] centroids or None when n < k."""
    n = _rows(vectors, dim)
    v, pv = _ptr(vectors, np.float32)
    out = _empty_like(vectors, (k, dim), np.float32)
    o, po = _ptr(out, np.float32)
    produced = C.c_int32(0)
    check(ctx._lib.vg_kmeans_train(ctx._h, pv, C.c_int64(n), C.c_int32(dim), C.c_int32(k), C.c_int32(int(metric)),
                                   C.c_int32(max_iter), C.c_uint64(seed), po, C.byref(produced),
                                   _stream_ptr(stream)))
    return out if produced.value else None


def kmeans_assign(ctx: Context, vectors, centroids, dim: int, metric=0, stream=None):
    """kmeans.AssignPartition (kmeans.go:142-196), batched."""
    n = _rows(vectors, dim)
    k = _rows(centroids, dim)
    v, pv = _ptr(vectors, np.float32)
    c, pc = _ptr(centroids, np.float32)
    out = _empty_like(vectors, (n,), np.int32)
    o, po = _ptr(out, np.int32, n)
    check(ctx._lib.vg_kmeans_assign(ctx._h, pv, C.c_int64(n), C.c_int32(dim), pc, C.c_int32(k),
                                    C.c_int32(int(metric)), po, _stream_ptr(stream)))
    return out


def find_closest_centroids(ctx: Context, query, centroids, dim: int, nprobe: int, metric=0, stream=None):
    """kmeans.FindClosestCentroids (kmeans.go:217-280)."""
    k = _rows(centroids, dim)
    q = np.ascontiguousarray(query, np.float32)
    c = np.ascontiguousarray(centroids, np.float32)
    out = np.empty(max(min(nprobe, k), 1), np.int32)
    n_out = C.c_int32(0)
    check(ctx._lib.vg_find_closest_centroids(ctx._h, C.c_void_p(q.ctypes.data), C.c_void_p(c.ctypes.data),
                                             C.c_int32(dim), C.c_int32(k), C.c_int32(nprobe),
                                             C.c_int32(int(metric)), C.c_void_p(out.ctypes.data),
                                             C.byref(n_out), _stream_ptr(stream)))
    return out[:n_out.value]


class RaBitQuantizer:
    """quantization.RaBitQuantizer (internal/quantization/rabitq.go:26-49)."""

    def __init__(self, ctx: Context, dimension: int):
        if dimension <= 0:
            raise VecgoHipError(-1, "dimension must be positive")
        self.ctx, self.dimension = ctx, dimension
        self._lib = ctx._lib
        self._lib.vg_rabitq_code_bytes.restype = C.c_int64

    def bytes_total(self) -> int:
        """BytesTotal (rabitq.go:187-190)."""
        return int(self._lib.vg_rabitq_code_bytes(C.c_int32(self.dimension)))

    def encode(self, vectors, out=None, stream=None):
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        if out is None:
            out = _empty_like(vectors, (n, self.bytes_total()), np.uint8)
        c, pc = _ptr(out, np.uint8, n * self.bytes_total())
        check(self._lib.vg_rabitq_encode(self.ctx._h, C.c_int32(self.dimension), pv, C.c_int64(n), pc,
                                         _stream_ptr(stream)))
        return out

    def distance(self, query, codes, out=None, stream=None):
        """Distance (rabitq.go:119-176) of one query against n codes."""
        if _rows(query, self.dimension) != 1:
            raise VecgoHipError(-2, "vector dimension mismatch")
        total = codes.numel() if _is_torch(codes) else np.asarray(codes).size
        if total % self.bytes_total():
            raise VecgoHipError(-4, "invalid code length")
        n = total // self.bytes_total()
        q, pq_ = _ptr(query, np.float32)
        c, pc = _ptr(codes, np.uint8)
        if out is None:
            out = _empty_like(codes, (n,), np.float32)
        o, po = _ptr(out, np.float32, n)
        check(self._lib.vg_rabitq_distance_batch(self.ctx._h, C.c_int32(self.dimension), pq_, pc,
                                                 C.c_int64(n), po, _stream_ptr(stream)))
        return out


class ScalarQuantizer:
    """quantization.ScalarQuantizer (internal/quantization/quantizer.go:27-39): 8 bits per
    dimension, per-dimension min / max."""

    def __init__(self, ctx: Context, dimension: int):
        self.ctx, self.dimension = ctx, dimension
        self._lib = ctx._lib
        h = C.c_void_p()
        check(self._lib.vg_sq8_create(ctx._h, C.c_int32(dimension), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vg_sq8_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def is_trained(self) -> bool:
        return bool(self._lib.vg_sq8_is_trained(self._h))

    def bytes_per_dimension(self) -> int:
        return 1

    def compression_ratio(self) -> float:
        return 4.0

    def train(self, vectors, stream=None):
        """Train (quantizer.go:127-180)."""
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        check(self._lib.vg_sq8_train(self._h, pv, C.c_int64(n), _stream_ptr(stream)))

    def set_bounds(self, mins, maxs):
        """SetBounds (quantizer.go:52-78)."""
        a, pa = _ptr(mins, np.float32, self.dimension)
        b, pb = _ptr(maxs, np.float32, self.dimension)
        check(self._lib.vg_sq8_set_bounds(self._h, pa, pb))

    def params(self):
        """(mins, maxs, scales, inv_scales) as numpy arrays."""
        out = [np.empty(self.dimension, np.float32) for _ in range(4)]
        check(self._lib.vg_sq8_get_params(self._h, *[C.c_void_p(a.ctypes.data) for a in out]))
        return tuple(out)

    def encode(self, vectors, out=None, stream=None):
        """Encode (quantizer.go:183-222), batched: returns [n, dim] uint8."""
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        if out is None:
            out = _empty_like(vectors, (n, self.dimension), np.uint8)
        c, pc = _ptr(out, np.uint8, n * self.dimension)
        check(self._lib.vg_sq8_encode(self._h, pv, C.c_int64(n), pc, _stream_ptr(stream)))
        return out

    def decode(self, codes, out=None, stream=None):
        """Decode (quantizer.go:225-250), batched: returns [n, dim] float32."""
        total = codes.numel() if _is_torch(codes) else np.asarray(codes).size
        if total % self.dimension:
            raise VecgoHipError(-2, "vector dimension mismatch")
        n = total // self.dimension
        c, pc = _ptr(codes, np.uint8)
        if out is None:
            out = _empty_like(codes, (n, self.dimension), np.float32)
        o, po = _ptr(out, np.float32, n * self.dimension)
        check(self._lib.vg_sq8_decode(self._h, pc, C.c_int64(n), po, _stream_ptr(stream)))
        return out

    def l2_distance_batch(self, query, codes, out=None, stream=None):
        """L2DistanceBatch (quantizer.go:93-106): one query against n codes."""
        if _rows(query, self.dimension) != 1:
            raise VecgoHipError(-2, "query dimension mismatch")
        total = codes.numel() if _is_torch(codes) else np.asarray(codes).size
        n = total // self.dimension
        q, pq_ = _ptr(query, np.float32)
        c, pc = _ptr(codes, np.uint8)
        if out is None:
            out = _empty_like(codes, (n,), np.float32)
        o, po = _ptr(out, np.float32, n)
        check(self._lib.vg_sq8_l2_distance_batch(self._h, pq_, pc, C.c_int64(n), po, _stream_ptr(stream)))
        return out


class Int4Quantizer:
    """quantization.Int4Quantizer (internal/quantization/int4.go:12-20): 4 bits per dimension."""

    def __init__(self, ctx: Context, dimension: int):
        self.ctx, self.dimension = ctx, dimension
        self._lib = ctx._lib
        self._lib.vg_int4_code_bytes.restype = C.c_int64
        h = C.c_void_p()
        check(self._lib.vg_int4_create(ctx._h, C.c_int32(dimension), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vg_int4_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def is_trained(self) -> bool:
        return bool(self._lib.vg_int4_is_trained(self._h))

    @property
    def code_bytes(self) -> int:
        return (self.dimension + 1) // 2

    def bytes_per_dimension(self) -> int:
        return 0  # sub-byte (int4.go:167-169)

    def train(self, vectors, stream=None):
        """Train (int4.go:29-62)."""
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        check(self._lib.vg_int4_train(self._h, pv, C.c_int64(n), _stream_ptr(stream)))

    def set_params(self, min_val, diff):
        """UnmarshalBinary (int4.go:190-219)."""
        a, pa = _ptr(min_val, np.float32, self.dimension)
        b, pb = _ptr(diff, np.float32, self.dimension)
        check(self._lib.vg_int4_set_params(self._h, pa, pb))

    def params(self):
        """(min, diff, lookup table[dim*16]) as numpy arrays."""
        mn, df = np.empty(self.dimension, np.float32), np.empty(self.dimension, np.float32)
        tb = np.empty(self.dimension * 16, np.float32)
        check(self._lib.vg_int4_get_params(self._h, C.c_void_p(mn.ctypes.data), C.c_void_p(df.ctypes.data),
                                           C.c_void_p(tb.ctypes.data)))
        return mn, df, tb

    def encode(self, vectors, out=None, stream=None):
        """Encode (int4.go:65-105), batched: returns [n, ceil(dim/2)] uint8."""
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        if out is None:
            out = _empty_like(vectors, (n, self.code_bytes), np.uint8)
        c, pc = _ptr(out, np.uint8, n * self.code_bytes)
        check(self._lib.vg_int4_encode(self._h, pv, C.c_int64(n), pc, _stream_ptr(stream)))
        return out

    def decode(self, codes, out=None, stream=None):
        """Decode (int4.go:108-130), batched: returns [n, dim] float32."""
        total = codes.numel() if _is_torch(codes) else np.asarray(codes).size
        if total % self.code_bytes:
            raise VecgoHipError(-2, "dimension mismatch")
        n = total // self.code_bytes
        c, pc = _ptr(codes, np.uint8)
        if out is None:
            out = _empty_like(codes, (n, self.dimension), np.float32)
        o, po = _ptr(out, np.float32, n * self.dimension)
        check(self._lib.vg_int4_decode(self._h, pc, C.c_int64(n), po, _stream_ptr(stream)))
        return out

    def _dist(self, query, codes, precomputed, out, stream):
        if _rows(query, self.dimension) != 1:
            raise VecgoHipError(-2, "dimension mismatch")
        total = codes.numel() if _is_torch(codes) else np.asarray(codes).size
        n = total // self.code_bytes
        q, pq_ = _ptr(query, np.float32)
        c, pc = _ptr(codes, np.uint8)
        if out is None:
            out = _empty_like(codes, (n,), np.float32)
        o, po = _ptr(out, np.float32, n)
        check(self._lib.vg_int4_l2_distance_batch(self._h, pq_, pc, C.c_int64(n), C.c_int32(precomputed), po,
                                                  _stream_ptr(stream)))
        return out

    def l2_distance_batch(self, query, codes, out=None, stream=None):
        """L2DistanceBatch (int4.go:150-164)."""
        return self._dist(query, codes, 0, out, stream)

    def l2_distance(self, query, codes, out=None, stream=None):
        """L2Distance (int4.go:133-147) of one query against each of n codes."""
        return self._dist(query, codes, 1, out, stream)

    SCAN_KERNELS = ("tab", "pair128", "pair_tail", "row")   # Int4ScanKernel, csrc/vg_int4_plan.hpp

    def scan_plan(self, n: int, codes_aligned16: bool = True) -> dict:
        """What l2_distance / l2_distance_batch would launch over n rows (vg_int4_scan_plan; nothing runs): the kernel's name,
        waves per workgroup, workgroups and dynamic LDS bytes."""
        plan = (C.c_int64 * 4)()
        check(self._lib.vg_int4_scan_plan(self._h, C.c_int64(n), C.c_int32(1 if codes_aligned16 else 0), plan))
        return {"kernel": self.SCAN_KERNELS[plan[0]], "waves": int(plan[1]), "blocks": int(plan[2]), "lds": int(plan[3])}


def hamming_batch(ctx: Context, a, codes, out=None, stream=None):
    """simd.Hamming (kernels.go:71) of one byte string against n contiguous ones."""
    a_, pa = _ptr(a, np.uint8)
    nbytes = a_.numel() if _is_torch(a_) else a_.size
    total = codes.numel() if _is_torch(codes) else np.asarray(codes).size
    n = total // nbytes if nbytes else 0
    c, pc = _ptr(codes, np.uint8)
    if out is None:
        out = _empty_like(codes, (n,), np.int32)
    o, po = _ptr(out, np.int32, n)
    check(ctx._lib.vg_hamming_batch(ctx._h, pa, pc, C.c_int64(nbytes), C.c_int64(n), po, _stream_ptr(stream)))
    return out


class ProductQuantizer:
    """quantization.ProductQuantizer (internal/quantization/pq.go:20-29)."""

    def __init__(self, ctx: Context, dimension: int, num_subvectors: int, num_centroids: int = 256):
        self._lib = ctx._lib
        self.ctx = ctx
        h = C.c_void_p()
        check(self._lib.vg_pq_create(ctx._h, dimension, num_subvectors, num_centroids, C.byref(h)))
        self._h = h
        self.dimension, self.num_subvectors, self.num_centroids = dimension, num_subvectors, num_centroids
        self.subvector_dim = dimension // num_subvectors

    @classmethod
    def _borrowed(cls, ctx: Context, handle, dimension: int, num_subvectors: int, num_centroids: int, owner):
        """A view of a quantizer another object owns (the inner PQ of an OptimizedProductQuantizer)."""
        self = cls.__new__(cls)
        self._lib, self.ctx, self._h, self._owner = ctx._lib, ctx, handle, owner
        self.dimension, self.num_subvectors, self.num_centroids = dimension, num_subvectors, num_centroids
        self.subvector_dim = dimension // num_subvectors
        return self

    def close(self):
        if getattr(self, "_h", None) and getattr(self, "_owner", None) is None:
            self._lib.vg_pq_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def is_trained(self) -> bool:
        return bool(self._lib.vg_pq_is_trained(self._h))

    def set_codebooks(self, codebooks, scales, offsets):
        n = self.num_subvectors * self.num_centroids * self.subvector_dim
        a, pa = _ptr(codebooks, np.int8, n)
        s, ps = _ptr(scales, np.float32, self.num_subvectors)
        o, po = _ptr(offsets, np.float32, self.num_subvectors)
        check(self._lib.vg_pq_set_codebooks(self._h, pa, ps, po))

    def codebooks(self):
        n = self.num_subvectors * self.num_centroids * self.subvector_dim
        cb = np.empty(n, np.int8); s = np.empty(self.num_subvectors, np.float32)
        o = np.empty(self.num_subvectors, np.float32)
        check(self._lib.vg_pq_get_codebooks(self._h, C.c_void_p(cb.ctypes.data),
                                            C.c_void_p(s.ctypes.data), C.c_void_p(o.ctypes.data)))
        return cb, s, o

    def train(self, vectors, iters: int = 20, seed: int = 1, stream=None):
        """Train (pq.go:68-143); the reference uses 20 Lloyd iterations."""
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        check(self._lib.vg_pq_train(self._h, pv, C.c_int64(n), C.c_int32(iters), C.c_uint64(seed),
                                    _stream_ptr(stream)))

    def train_subset(self, vectors, sub_begin: int, sub_count: int, iters: int = 20, seed: int = 1, stream=None):
        """Train only the sub-quantizers [sub_begin, sub_begin + sub_count) (the reference trains
        them as independent goroutines, pq.go:83-138); see vecgo_amd.sharded.train_pq_sharded."""
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        check(self._lib.vg_pq_train_subset(self._h, pv, C.c_int64(n), C.c_int32(iters), C.c_uint64(seed),
                                           C.c_int32(sub_begin), C.c_int32(sub_count), _stream_ptr(stream)))

    def codebooks_range(self, sub_begin: int, sub_count: int):
        per = self.num_centroids * self.subvector_dim
        cb = np.empty(sub_count * per, np.int8); s = np.empty(sub_count, np.float32)
        o = np.empty(sub_count, np.float32)
        check(self._lib.vg_pq_get_codebooks_range(self._h, C.c_int32(sub_begin), C.c_int32(sub_count),
                                                  C.c_void_p(cb.ctypes.data), C.c_void_p(s.ctypes.data),
                                                  C.c_void_p(o.ctypes.data)))
        return cb, s, o

    def encode(self, vectors, out=None, stream=None):
        """Encode (pq.go:147-176), batched: returns [n, m] uint8."""
        n = _rows(vectors, self.dimension)
        v, pv = _ptr(vectors, np.float32)
        if out is None:
            out = _empty_like(vectors, (n, self.num_subvectors), np.uint8)
        c, pc = _ptr(out, np.uint8, n * self.num_subvectors)
        check(self._lib.vg_pq_encode(self._h, pv, C.c_int64(n), pc, _stream_ptr(stream)))
        return out

    def decode(self, codes, out=None, stream=None):
        """Decode (pq.go:185-229), batched: returns [n, dim] float32."""
        total = codes.numel() if _is_torch(codes) else np.asarray(codes).size
        if total % self.num_subvectors:
            raise VecgoHipError(-4, "invalid code length")
        n = total // self.num_subvectors
        c, pc = _ptr(codes, np.uint8)
        if out is None:
            out = _empty_like(codes, (n, self.dimension), np.float32)
        o, po = _ptr(out, np.float32, n * self.dimension)
        check(self._lib.vg_pq_decode(self._h, pc, C.c_int64(n), po, _stream_ptr(stream)))
        return out

    def asymmetric_distance(self, query, codes, out=None, stream=None):
        """ComputeAsymmetricDistance (pq.go:234-260) of one query against n codes."""
        if _rows(query, self.dimension) != 1:
            raise VecgoHipError(-2, "vector dimension mismatch")
        total = codes.numel() if _is_torch(codes) else np.asarray(codes).size
        if total % self.num_subvectors:
            raise VecgoHipError(-4, "codes length mismatch")
        n = total // self.num_subvectors
        q, pq_ = _ptr(query, np.float32)
        c, pc = _ptr(codes, np.uint8)
        if out is None:
            out = _empty_like(codes, (n,), np.float32)
        o, po = _ptr(out, np.float32, n)
        check(self._lib.vg_pq_asymmetric_distance_batch(self._h, pq_, pc, C.c_int64(n), po,
                                                        _stream_ptr(stream)))
        return out

    def build_distance_table(self, queries, out=None, stream=None):
        """BuildDistanceTable (pq.go:468-491), batched: returns [nq, m*k]."""
        nq = _rows(queries, self.dimension)
        q, pq_ = _ptr(queries, np.float32)
        if out is None:
            out = _empty_like(queries, (nq, self.num_subvectors * self.num_centroids), np.float32)
        t, pt = _ptr(out, np.float32, nq * self.num_subvectors * self.num_centroids)
        check(self._lib.vg_pq_build_distance_table(self._h, pq_, C.c_int64(nq), pt, _stream_ptr(stream)))
        return out


def _rows(x, dim) -> int:
    n = x.numel() if _is_torch(x) else np.asarray(x).size
    if dim <= 0 or n % dim:
        raise VecgoHipError(-2, "vector dimension mismatch")
    return n // dim


def _empty_like(ref, shape, dtype):
    if _is_torch(ref):
        tdt = {np.float32: torch.float32, np.uint32: torch.int32, np.uint8: torch.uint8,
               np.int32: torch.int32}[dtype]
        return torch.empty(shape, dtype=tdt, device=ref.device)
    return np.empty(shape, dtype)


class Index:
    """Device-resident rows / codes / graph of one segment."""

    def __init__(self, ctx: Context, n: int, dim: int, metric: Metric = Metric.L2):
        self._lib = ctx._lib
        self.ctx = ctx
        h = C.c_void_p()
        check(self._lib.vg_index_create(ctx._h, C.c_int64(n), dim, int(metric), C.byref(h)))
        self._h = h
        self.n, self.dim, self.metric = n, dim, Metric(metric)
        self._keep = []

    @classmethod
    def _borrowed(cls, ctx: Context, handle, n: int, dim: int, metric: int, owner):
        """An Index view of a handle owned by something else (a Segment)."""
        self = cls.__new__(cls)
        self._lib, self.ctx, self._h = ctx._lib, ctx, handle
        self.n, self.dim, self.metric = n, dim, Metric(metric)
        self._keep = [owner]
        self._borrowed_handle = True
        return self

    @classmethod
    def _adopted(cls, ctx: Context, handle, n: int, dim: int, metric: int):
        """An Index that owns a handle the library created (vg_index_merge): closed like one made by __init__."""
        self = cls.__new__(cls)
        self._lib, self.ctx, self._h = ctx._lib, ctx, handle
        self.n, self.dim, self.metric = n, dim, Metric(metric)
        self._keep = []
        return self

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed_handle", False):
                self._lib.vg_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_pq_codes(self, pq: ProductQuantizer, codes, stream=None):
        c, pc = _ptr(codes, np.uint8, self.n * pq.num_subvectors)
        self._keep.append(pq)
        check(self._lib.vg_index_set_pq_codes(self._h, pq._h, pc, _stream_ptr(stream)))

    def set_sq8_codes(self, sq: "ScalarQuantizer", codes, stream=None):
        c, pc = _ptr(codes, np.uint8, self.n * self.dim)
        self._keep.append(sq)
        check(self._lib.vg_index_set_sq8_codes(self._h, sq._h, pc, _stream_ptr(stream)))

    def set_int4_codes(self, iq: "Int4Quantizer", codes, stream=None):
        c, pc = _ptr(codes, np.uint8, self.n * iq.code_bytes)
        self._keep.append(iq)
        check(self._lib.vg_index_set_int4_codes(self._h, iq._h, pc, _stream_ptr(stream)))

    def search_int4(self, queries, k, mask=None, out=None, stream=None):
        """Exhaustive scan of the INT4 codes (vg_search_int4): Int4Quantizer.L2Distance (int4.go:136-147) per row — the bits
        l2_distance gives the row and search_vamana(kind=3) reports for it —, the k best by (Score, RowID), scores ascending
        whatever the metric.  mask: as search_flat_filtered's (bool[n] / packed bits for the batch, bool[nq, n] / packed
        [nq, stride >= ceil(n/8)] for one filter per query; None = every row).  k <= 512."""
        m, pm, stride = (None, None, 0) if mask is None else self._packed_mask(mask, _rows(queries, self.dim), "search_int4")
        return self._search(self._lib.vg_search_int4, queries, k, extra=(pm, C.c_int64(stride)), out=out, stream=stream)

    def set_partitions(self, centroids, part_offsets, stream=None):
        """IVF partitions of a flat segment (flat/segment.go:187-207): centroids [P, dim] fp32 and the
        first row of every partition [P + 1] uint32; None / empty removes them."""
        if centroids is None or len(part_offsets) == 0:
            check(self._lib.vg_index_set_partitions(self._h, None, None, C.c_int32(0), _stream_ptr(stream)))
            return
        c = np.ascontiguousarray(centroids, np.float32).reshape(-1, self.dim)
        o = np.ascontiguousarray(part_offsets, np.uint32)
        if o.size != c.shape[0] + 1:
            raise ValueError("part_offsets must have one entry more than there are centroids")
        check(self._lib.vg_index_set_partitions(self._h, C.c_void_p(c.ctypes.data), C.c_void_p(o.ctypes.data),
                                                C.c_int32(c.shape[0]), _stream_ptr(stream)))

    SCAN_F32, SCAN_PQ, SCAN_SQ8 = 0, 1, 2

    def search_flat_probed(self, queries, k, nprobes=0, scan=0, out=None, stream=None):
        """flat.Segment.Search over the nprobes closest IVF partitions (flat/segment.go:727-749)."""
        return self._search(self._lib.vg_search_flat_probed, queries, k, extra=(C.c_int32(nprobes), C.c_int32(scan)),
                            out=out, stream=stream)

    def search_flat_filtered(self, queries, k, mask, nprobes=0, scan=0, out=None, stream=None):
        """flat.Segment.Search with a row filter (flat/segment.go:631-635, :559-561): the k best (score, row id) among the
        rows whose mask entry is set, over the probed partitions or the whole segment.  mask: bool[n] / packed bits for the
        batch, or bool[nq, n] / packed [nq, ceil(n/8)] for one filter per query; None = search_flat_probed."""
        if mask is None:
            return self.search_flat_probed(queries, k, nprobes, scan, out=out, stream=stream)
        m, pm, stride = self._packed_mask(mask, _rows(queries, self.dim), "search_flat_filtered")
        return self._search(self._lib.vg_search_flat_filtered, queries, k,
                            extra=(C.c_int32(nprobes), C.c_int32(scan), pm, C.c_int64(stride)),
                            out=out, stream=stream)

    def search_flat_prefilter(self, queries, k, mask, out=None, stream=None):
        """The engine's bitmap strategy over this segment (vg_search_flat_prefilter; engine/search.go:602-736): only the rows
        whose mask bit is set are fetched and scored (distance.SquaredL2 / Dot from the fp32 rows), the best k by (score, row
        id) are kept.  mask: as search_flat_filtered's (one for the batch or one per query; required).  IVF partitions are
        ignored: on an unpartitioned index the answer equals search_flat_filtered(..., scan=SCAN_F32) bit for bit.  The
        cost follows the rows the masks keep, so this is the call for selective filters (INTEGRATION.md has the crossover);
        it waits for the stream once.  k <= 16384."""
        if mask is None:
            raise ValueError("search_flat_prefilter: a mask is required (a search without a filter is search_flat)")
        m, pm, stride = self._packed_mask(mask, _rows(queries, self.dim), "search_flat_prefilter")
        return self._search(self._lib.vg_search_flat_prefilter, queries, k, extra=(pm, C.c_int64(stride)), out=out, stream=stream)

    def enable_pq_nomination(self, on: bool = True, stream=None):
        """vg_index_enable_pq_nomination: batches of search_pq_adc (queries x rows >= 24M, k <= 256, K = 256) are nominated by a bfloat16
        MFMA GEMM over the decoded rows (+ n * dim * 2 bytes), re-scored from the codes against the query's distance table in
        the reference's order and proven: ids and scores stay bit-identical."""
        check(self._lib.vg_index_enable_pq_nomination(self._h, C.c_int32(1 if on else 0), _stream_ptr(stream)))

    def enable_pq_nomination_from_codes(self, on: bool = True, stream=None):
        """vg_index_enable_pq_nomination_from_codes: the same nomination without the image of the decoded rows — the GEMM's row tiles
        are gathered from a bfloat16 copy of the decoded codebook by the rows' codes (8 dimensions per sub-quantizer, K = 256;
        batches above 128 queries, from queries x rows >= 13M).  Resident: 4 bytes a row and the codebook.  Exclusive with enable_pq_nomination; ids and
        scores stay bit-identical."""
        check(self._lib.vg_index_enable_pq_nomination_from_codes(self._h, C.c_int32(1 if on else 0), _stream_ptr(stream)))

    def pq_nomination_info(self):
        """vg_index_pq_nomination_info: (mode, held_bytes) — mode 0 off, 1 the decoded-row image, 2 from the codes; held_bytes the
        device memory the mode keeps resident."""
        mode, held = C.c_int32(0), C.c_int64(0)
        check(self._lib.vg_index_pq_nomination_info(self._h, C.byref(mode), C.byref(held)))
        return mode.value, held.value

    def enable_sq8_nomination(self, on: bool = True, stream=None):
        """vg_index_enable_sq8_nomination: batches of search_sq8 (L2 or Dot, 5 queries up, k <= 256, any dim) are nominated by a
        bfloat16 MFMA GEMM over the dequantised rows (+ n * dim * 2 bytes), re-scored exactly from the codes and proven: ids and
        scores stay bit-identical."""
        check(self._lib.vg_index_enable_sq8_nomination(self._h, C.c_int32(1 if on else 0), _stream_ptr(stream)))

    def enable_sq8_nomination_from_codes(self, on: bool = True, stream=None):
        """vg_index_enable_sq8_nomination_from_codes: the same nomination without the image of the dequantised rows — the queries are
        scaled by the inverse scales and the GEMM's row tiles converted from the code tiles, bf16(code - 128), exact (whole-segment,
        unfiltered batches above 128 queries, from queries x rows >= 12M).  Resident: 4 bytes a row and 4 a dimension.  Exclusive
        with enable_sq8_nomination; ids and scores stay bit-identical."""
        check(self._lib.vg_index_enable_sq8_nomination_from_codes(self._h, C.c_int32(1 if on else 0), _stream_ptr(stream)))

    def sq8_nomination_info(self):
        """vg_index_sq8_nomination_info: (mode, held_bytes, rescanned) — mode 0 off, 1 the dequantised-row image, 2 from the codes;
        held_bytes the device memory the mode keeps resident; rescanned the queries whose proof failed since it was enabled."""
        mode, held, rescanned = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        check(self._lib.vg_index_sq8_nomination_info(self._h, C.byref(mode), C.byref(held), C.byref(rescanned)))
        return mode.value, held.value, rescanned.value

    def enable_rabitq_nomination(self, on: bool = True, stream=None):
        """vg_index_enable_rabitq_nomination: batches of search_rabitq above 128 queries (k <= 256, queries x rows >= 12M) are nominated by
        an int8 MFMA GEMM over the sign bits — the Hamming distances come out exact —, listed behind a conservative screen, re-scored
        with popcount and the reference's formula and proven; the others keep the scan.  Nothing resident; ids and scores stay
        bit-identical.  An index that holds a negative stored norm keeps the scan."""
        check(self._lib.vg_index_enable_rabitq_nomination(self._h, C.c_int32(1 if on else 0), _stream_ptr(stream)))

    def rabitq_nomination_info(self):
        """vg_index_rabitq_nomination_info: (on, held_bytes, rescanned, mismatched) — held_bytes the device memory the mode keeps
        resident (0); rescanned the queries whose list was incomplete and the scan answered since it was enabled; mismatched, under
        the test hook VG_RABITQ_NOM_CHECK, the listed keys whose Hamming distance was not the popcount's."""
        on, held, rescanned, mismatched = C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(self._lib.vg_index_rabitq_nomination_info(self._h, C.byref(on), C.byref(held), C.byref(rescanned), C.byref(mismatched)))
        return on.value, held.value, rescanned.value, mismatched.value

    def search_sq8(self, queries, k, out=None, stream=None):
        """flat.Segment.Search SQ8 branch (flat/segment.go:517-604)."""
        return self._search(self._lib.vg_search_sq8, queries, k, out=out, stream=stream)

    def set_rabitq_codes(self, codes, stream=None):
        lib = self._lib
        lib.vg_rabitq_code_bytes.restype = C.c_int64
        cb = int(lib.vg_rabitq_code_bytes(C.c_int32(self.dim)))
        c, pc = _ptr(codes, np.uint8, self.n * cb)
        check(lib.vg_index_set_rabitq_codes(self._h, pc, _stream_ptr(stream)))

    def search_rabitq(self, queries, k, out=None, stream=None):
        """Exhaustive RaBitQ scan (rabitq.go:119-176 per row), top-k by (Score, RowID)."""
        return self._search(self._lib.vg_search_rabitq, queries, k, out=out, stream=stream)

    def set_hnsw_graph(self, l0, upper=(), entry_point=0, m=None, stream=None):
        """l0: [n, m0] uint32 (0xFFFFFFFF terminates a list); upper: list of (slot[n], adj[rows, m])
        for levels 1..L."""
        l0a = np.ascontiguousarray(l0, np.uint32)
        m0 = l0a.shape[1]
        L = len(upper)
        if L:
            m_ = upper[0][1].shape[1]
            slots = np.ascontiguousarray(np.stack([np.asarray(s_, np.uint32) for s_, _ in upper]))
            adj = np.ascontiguousarray(np.concatenate([np.asarray(a, np.uint32).reshape(-1, m_) for _, a in upper]))
            rows = np.array([np.asarray(a).reshape(-1, m_).shape[0] for _, a in upper], np.int64)
            ps, pa, pr = (C.c_void_p(slots.ctypes.data), C.c_void_p(adj.ctypes.data),
                          C.c_void_p(rows.ctypes.data))
        else:
            m_ = m if m is not None else max(1, m0 // 2)
            ps = pa = pr = None
        check(self._lib.vg_index_set_hnsw_graph(self._h, C.c_int32(m0), C.c_void_p(l0a.ctypes.data),
                                                C.c_int32(L), C.c_int32(m_), ps, pa, pr,
                                                C.c_uint32(entry_point), _stream_ptr(stream)))

    def build_hnsw(self, m=32, ef_construction=300, max_batch=8192, growth_div=32, stream=None):
        """hnsw.Insert over rows 0..n-1 on the GPU (hnsw.go:713-984; ids and levels of ApplyInsert); the
        graph becomes the index's HNSW graph.  max_batch=1 is the reference's sequential loop."""
        check(self._lib.vg_hnsw_build(self._h, C.c_int32(m), C.c_int32(ef_construction), C.c_int32(max_batch),
                                      C.c_int32(growth_div), _stream_ptr(stream)))

    def insert_hnsw(self, rows, m=32, ef_construction=300, max_batch=8192, growth_div=32, stream=None):
        """hnsw.ApplyInsert on the GPU (vg_hnsw_insert): rows [count, dim] fp32 are appended as rows n .. n+count-1 and
        linked into the index's HNSW graph (ids = row numbers, levels of ApplyInsert; batches of clamp(inserted /
        growth_div, 1, max_batch)).  An empty index (n = 0) gets its rows and graph from the first call."""
        if not _is_torch(rows):
            rows = np.asarray(rows)
        shape = tuple(rows.shape)
        if len(shape) != 2 or shape[1] != self.dim:
            raise ValueError(f"insert_hnsw: rows must be [count, {self.dim}], got {shape}")
        if (rows.dtype != torch.float32) if _is_torch(rows) else (np.asarray(rows).dtype != np.float32):
            raise TypeError(f"insert_hnsw: rows must be float32, got {rows.dtype}")
        count = shape[0]
        r, pr = _ptr(rows, np.float32, count * self.dim)
        check(self._lib.vg_hnsw_insert(self._h, pr, C.c_int64(count), C.c_int32(m), C.c_int32(ef_construction),
                                       C.c_int32(max_batch), C.c_int32(growth_div), _stream_ptr(stream)))
        self.n += count

    def compact_hnsw(self, ef_construction=300, max_batch=8192, stream=None):
        """hnsw.Compact on the GPU (vg_hnsw_compact) under the tombstones of set_hnsw_tombstones: live nodes whose lists
        are mostly dead are repaired (batches of max_batch nodes in id order; max_batch=1 is the reference with one worker),
        live nodes' lists lose their tombstoned ids, tombstoned nodes' lists are emptied.  Returns the counters
        {repaired_nodes, repaired_lists, pruned_links, cleared_nodes}."""
        if isinstance(ef_construction, bool) or not isinstance(ef_construction, (int, np.integer)):
            raise TypeError(f"compact_hnsw: ef_construction must be an int, got {type(ef_construction).__name__}")
        if isinstance(max_batch, bool) or not isinstance(max_batch, (int, np.integer)):
            raise TypeError(f"compact_hnsw: max_batch must be an int, got {type(max_batch).__name__}")
        if ef_construction < 0 or ef_construction > 1024:
            raise ValueError(f"compact_hnsw: ef_construction must be in 0..1024 (0 = 300), got {ef_construction}")
        if max_batch < 1:
            raise ValueError(f"compact_hnsw: max_batch must be >= 1, got {max_batch}")
        stats = (C.c_int64 * 4)()
        check(self._lib.vg_hnsw_compact(self._h, C.c_int32(ef_construction), C.c_int32(max_batch), stats, _stream_ptr(stream)))
        return dict(zip(("repaired_nodes", "repaired_lists", "pruned_links", "cleared_nodes"), (int(v) for v in stats)))

    def get_hnsw_graph(self, stream=None):
        """(l0[n, m0], upper=[(slot[n], adj[rows, m])...], entry_point) — set_hnsw_graph's arguments."""
        m0, m_, L, ep = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint32()
        rows = np.zeros(64, np.int64)
        sp = _stream_ptr(stream)
        check(self._lib.vg_index_get_hnsw_graph(self._h, C.byref(m0), C.byref(m_), C.byref(L), C.byref(ep),
                                                C.c_void_p(rows.ctypes.data), None, None, None, sp))
        L = L.value
        rows = rows[:L]
        l0 = np.empty((self.n, m0.value), np.uint32)
        slots = np.empty((max(L, 1), self.n), np.uint32)
        adj = np.empty((max(int(rows.sum()), 1), m_.value), np.uint32)
        check(self._lib.vg_index_get_hnsw_graph(self._h, None, None, None, None, None, C.c_void_p(l0.ctypes.data),
                                                C.c_void_p(slots.ctypes.data), C.c_void_p(adj.ctypes.data), sp))
        upper, off = [], 0
        for l in range(L):
            upper.append((slots[l].copy(), adj[off:off + int(rows[l])].copy()))
            off += int(rows[l])
        return l0, upper, int(ep.value)

    def set_vamana_graph(self, graph, entry_point, stream=None):
        g = np.ascontiguousarray(graph, np.uint32)
        check(self._lib.vg_index_set_vamana_graph(self._h, C.c_int32(g.shape[1]), C.c_void_p(g.ctypes.data),
                                                  C.c_uint32(entry_point), _stream_ptr(stream)))

    def build_vamana(self, r=64, l=100, alpha=1.2, init_graph=None, seed=0, max_batch=8192, growth_div=32, stream=None):
        """diskann.Writer.buildGraph over rows 0..n-1 on the GPU (diskann/writer.go:362-460; the rules are
        vg_vamana_build's in the header); the graph becomes the index's Vamana graph.  init_graph: [n, r] ids
        (0xFFFFFFFF = empty slot) or None for the seeded random start.  max_batch=1 is the writer's sequential loop."""
        g = None
        if init_graph is not None:
            g = np.ascontiguousarray(init_graph, np.uint32)
            if g.shape != (self.n, r):
                raise ValueError(f"init_graph must be [{self.n}, {r}], got {g.shape}")
        check(self._lib.vg_vamana_build(self._h, C.c_int32(r), C.c_int32(l), C.c_float(alpha),
                                        None if g is None else C.c_void_p(g.ctypes.data), C.c_uint64(seed),
                                        C.c_int32(max_batch), C.c_int32(growth_div), _stream_ptr(stream)))

    def insert_vamana(self, rows, r=64, l=100, alpha=1.2, deleted=None, seed=0, max_batch=8192, growth_div=32, stream=None):
        """FreshVamana.Insert on the GPU (vg_vamana_insert; the rules are the header's): rows [count, dim] fp32 are appended as
        rows n .. n+count-1 and linked into the index's Vamana graph (batches of clamp(nodes / growth_div, 1, max_batch);
        max_batch=1 is the reference's serialized loop).  deleted: bool[n] / packed bits over the rows before the call, or
        None.  An empty index (n = 0) gets its rows and graph from the first call."""
        if not _is_torch(rows):
            rows = np.asarray(rows)
        shape = tuple(rows.shape)
        if len(shape) != 2 or shape[1] != self.dim:
            raise ValueError(f"insert_vamana: rows must be [count, {self.dim}], got {shape}")
        if (rows.dtype != torch.float32) if _is_torch(rows) else (np.asarray(rows).dtype != np.float32):
            raise TypeError(f"insert_vamana: rows must be float32, got {rows.dtype}")
        count = shape[0]
        rr, pr = _ptr(rows, np.float32, count * self.dim)
        d, pd, _ = (None, None, 0) if deleted is None or self.n == 0 else self._packed_mask(deleted, 1, "insert_vamana")
        check(self._lib.vg_vamana_insert(self._h, pr, C.c_int64(count), C.c_int32(r), C.c_int32(l), C.c_float(alpha), pd,
                                         C.c_uint64(seed), C.c_int32(max_batch), C.c_int32(growth_div), _stream_ptr(stream)))
        self.n += count

    def consolidate_vamana(self, deleted, l=100, alpha=1.2, max_batch=8192, stream=None):
        """FreshVamana.consolidate on the GPU (vg_vamana_consolidate; the rules are the header's): every live node whose
        list names a deleted node is searched for and pruned again (batches of max_batch such nodes in id order; max_batch=1
        is the reference's loop); no reverse edges, the entry point stays.  deleted: bool[n] / packed bits, or None (nothing
        to do).  Returns the counters {repaired_nodes, dropped_links, links_before, links_after}."""
        if isinstance(l, bool) or not isinstance(l, (int, np.integer)):
            raise TypeError(f"consolidate_vamana: l must be an int, got {type(l).__name__}")
        if isinstance(max_batch, bool) or not isinstance(max_batch, (int, np.integer)):
            raise TypeError(f"consolidate_vamana: max_batch must be an int, got {type(max_batch).__name__}")
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)):
            raise TypeError(f"consolidate_vamana: alpha must be a number, got {type(alpha).__name__}")
        if l < 0 or l > 1024:
            raise ValueError(f"consolidate_vamana: l must be in 0..1024 (0 = 100), got {l}")
        if max_batch < 1 or max_batch > 16384:
            raise ValueError(f"consolidate_vamana: max_batch must be in 1..16384, got {max_batch}")
        d, pd, _ = (None, None, 0) if deleted is None or self.n == 0 else self._packed_mask(deleted, 1, "consolidate_vamana")
        stats = (C.c_int64 * 4)()
        check(self._lib.vg_vamana_consolidate(self._h, C.c_int32(l), C.c_float(alpha), pd, C.c_int32(max_batch), stats,
                                              _stream_ptr(stream)))
        return dict(zip(("repaired_nodes", "dropped_links", "links_before", "links_after"), (int(v) for v in stats)))

    def search_vamana_fresh(self, queries, k, l=100, deleted=None, mask=None, stream=None):
        """FreshVamana.Search, and with a mask SearchWithFilter, on the GPU (vg_search_vamana_fresh): l = the index's search
        list size; deleted: bool[n] / packed bits or None; mask: as search_vamana_filtered's.  Returns (ids [nq, k], scores,
        counts [nq]): query q's rows are ids[q, :counts[q]], the rest padded with 0xFFFFFFFF / +-Inf."""
        nq = _rows(queries, self.dim)
        q, pq_ = _ptr(queries, np.float32)
        d, pd, _ = (None, None, 0) if deleted is None or self.n == 0 else self._packed_mask(deleted, 1, "search_vamana_fresh")
        m, pm, stride = (None, None, 0) if mask is None else self._packed_mask(mask, nq, "search_vamana_fresh")
        ids = _empty_like(queries, (nq, k), np.uint32)
        scores = _empty_like(queries, (nq, k), np.float32)
        counts = _empty_like(queries, (nq,), np.int32)
        i, pi = _ptr(ids, np.uint32, nq * k)
        s, ps = _ptr(scores, np.float32, nq * k)
        c, pc = _ptr(counts, np.int32, nq)
        check(self._lib.vg_search_vamana_fresh(self._h, pq_, C.c_int64(nq), C.c_int32(k), C.c_int32(l), pd, pm, C.c_int64(stride),
                                               pi, ps, pc, _stream_ptr(stream)))
        return ids, scores, counts

    def get_vamana_graph(self, stream=None):
        """(graph[n, r], entry_point) — set_vamana_graph's arguments."""
        r, ep = C.c_int32(), C.c_uint32()
        sp = _stream_ptr(stream)
        check(self._lib.vg_index_get_vamana_graph(self._h, C.byref(r), C.byref(ep), None, sp))
        g = np.empty((self.n, r.value), np.uint32)
        if g.size:
            check(self._lib.vg_index_get_vamana_graph(self._h, None, None, C.c_void_p(g.ctypes.data), sp))
        return g, int(ep.value)

    def reorder_vamana_bfs(self, stream=None):
        """diskann.Writer.reorderBFS on the GPU (diskann/reorder.go:14-157; the rules are vg_vamana_reorder_bfs's in the
        header): the graph, its entry point and every per-row array of the index move into BFS order.  Returns
        (perm, inv_perm), np.uint32 of length n: perm[new] = old, inv_perm[old] = new."""
        perm = np.empty(self.n, np.uint32)
        inv = np.empty(self.n, np.uint32)
        check(self._lib.vg_vamana_reorder_bfs(self._h, C.c_void_p(perm.ctypes.data), C.c_void_p(inv.ctypes.data),
                                              _stream_ptr(stream)))
        return perm, inv

    QUANT_NONE, QUANT_PQ, QUANT_SQ8 = 0, 1, 3   # VG_QUANT_*

    def flat_build(self, num_partitions, quantizer=None, seed=0, kmeans_iters=0, pq_iters=0, stream=None):
        """flat.Writer.Flush's partitioning and quantization on the GPU (flat/writer.go:99-223; the rules are vg_flat_build's
        in the header): k-means over the resident rows, the stable regrouping by partition, then `quantizer` — None, a
        ScalarQuantizer, or a ProductQuantizer(dim, m, 256) — trained on and applied to the reordered rows and attached.
        Returns (perm, inv_perm), np.uint32 of length n: perm[new] = old, inv_perm[old] = new."""
        perm = np.empty(self.n, np.uint32)
        inv = np.empty(self.n, np.uint32)
        kind, sq, pq, m = self.QUANT_NONE, None, None, 0
        if isinstance(quantizer, ScalarQuantizer):
            kind, sq = self.QUANT_SQ8, quantizer._h
        elif isinstance(quantizer, ProductQuantizer):
            kind, pq, m = self.QUANT_PQ, quantizer._h, quantizer.num_subvectors
        elif quantizer is not None:
            raise TypeError("quantizer must be None, a ScalarQuantizer or a ProductQuantizer")
        check(self._lib.vg_flat_build(self._h, C.c_int32(num_partitions), C.c_int32(kind), C.c_int32(m), C.c_int32(kmeans_iters),
                                      C.c_int32(pq_iters), C.c_uint64(seed), sq, pq, C.c_void_p(perm.ctypes.data),
                                      C.c_void_p(inv.ctypes.data), _stream_ptr(stream)))
        if quantizer is not None and self.n:
            self._keep.append(quantizer)
        return perm, inv

    def write_flat_segment(self, segment_id=0, ids=None, metadata=None, block_stats=None, stream=None) -> bytes:
        """The file flat.Writer.Flush writes for this index (flat/writer.go:312-470; vg_segment_write_flat), the body's
        CRC-32C computed on the GPU.  ids: uint64 per row in the index's order (None: 0 .. n-1); metadata / block_stats: the
        sections as the host serialised them (None: the writer's bytes for rows without documents)."""
        def section(b):
            if b is None:
                return None, None, C.c_int64(-1)
            a = np.frombuffer(bytes(b) or b"\0", np.uint8)
            return a, C.c_void_p(a.ctypes.data), C.c_int64(len(b))
        md, pmd, nmd = section(metadata)
        bs, pbs, nbs = section(block_stats)
        self._lib.vg_segment_flat_image_size.restype = C.c_int64
        size = self._lib.vg_segment_flat_image_size(self._h, nmd, nbs)
        if size < 0:
            check(-5)
        i, pi = (None, None) if ids is None else _ptr(np.ascontiguousarray(ids, np.uint64), np.uint64, self.n)
        image = np.empty(size, np.uint8)
        written = C.c_int64(0)
        check(self._lib.vg_segment_write_flat(self._h, C.c_uint64(segment_id), pi, pmd, nmd, pbs, nbs, C.c_void_p(image.ctypes.data),
                                              C.c_int64(size), C.byref(written), _stream_ptr(stream)))
        return image[:written.value].tobytes()

    QUANT_RABITQ, QUANT_INT4 = 5, 6   # VG_QUANT_*

    def diskann_build(self, r=64, l=100, alpha=1.2, quantizer=None, seed=0, pq_iters=0, max_batch=8192, growth_div=32, stream=None):
        """diskann.Writer.Write up to Flush on the GPU (diskann/writer.go:217-253; the rules are vg_diskann_build's in the
        header): `quantizer` — None, a ProductQuantizer(dim, m, 256), a RaBitQuantizer or an Int4Quantizer — trained on and
        applied to the rows in add order and attached, then build_vamana(r, l, alpha, seed=seed, ...), then
        reorder_vamana_bfs.  Returns (perm, inv_perm, quantization_used): np.uint32 of length n, perm[new] = old,
        inv_perm[old] = new, and the VG_QUANT_* kind of the codes now on the index (QUANT_NONE for a ProductQuantizer over
        fewer than 256 rows: trainPQ's rule)."""
        kind, pq, iq, m = self.QUANT_NONE, None, None, 0
        if isinstance(quantizer, ProductQuantizer):
            kind, pq, m = self.QUANT_PQ, quantizer._h, quantizer.num_subvectors
        elif isinstance(quantizer, RaBitQuantizer):
            kind = self.QUANT_RABITQ
        elif isinstance(quantizer, Int4Quantizer):
            kind, iq = self.QUANT_INT4, quantizer._h
        elif quantizer is not None:
            raise TypeError("quantizer must be None, a ProductQuantizer, a RaBitQuantizer or an Int4Quantizer")
        perm = np.empty(self.n, np.uint32)
        inv = np.empty(self.n, np.uint32)
        used = C.c_int32(0)
        check(self._lib.vg_diskann_build(self._h, C.c_int32(r), C.c_int32(l), C.c_float(alpha), C.c_int32(kind), C.c_int32(m),
                                         C.c_int32(pq_iters), C.c_uint64(seed), C.c_int32(max_batch), C.c_int32(growth_div), pq, iq,
                                         C.c_void_p(perm.ctypes.data), C.c_void_p(inv.ctypes.data), C.byref(used), _stream_ptr(stream)))
        if used.value in (self.QUANT_PQ, self.QUANT_INT4):
            self._keep.append(quantizer)
        return perm, inv, int(used.value)

    def write_diskann_segment(self, segment_id=0, search_list_size=0, compression_type=1, ids=None, metadata=None,
                              metadata_index=None, stream=None) -> bytes:
        """The file diskann.Writer.Flush writes for this index (diskann/writer.go:645-856; vg_segment_write_diskann), most of
        the body's CRC-32C computed on the GPU.  search_list_size: the header's L (0 = 100); compression_type: recorded, the
        sections are raw; ids: uint64 per row in the index's order (None: 0 .. n-1); metadata / metadata_index: the sections as
        the host serialised them (None: the writer's bytes for rows without documents)."""
        def section(b):
            if b is None:
                return None, None, C.c_int64(-1)
            a = np.frombuffer(bytes(b) or b"\0", np.uint8)
            return a, C.c_void_p(a.ctypes.data), C.c_int64(len(b))
        md, pmd, nmd = section(metadata)
        mi, pmi, nmi = section(metadata_index)
        self._lib.vg_segment_diskann_image_size.restype = C.c_int64
        size = self._lib.vg_segment_diskann_image_size(self._h, nmd, nmi)
        i, pi = (None, None) if ids is None else _ptr(np.ascontiguousarray(ids, np.uint64), np.uint64, self.n)
        image = np.empty(max(size, 1), np.uint8)   # (size < 0: the call below names the refusal)
        written = C.c_int64(0)
        check(self._lib.vg_segment_write_diskann(self._h, C.c_uint64(segment_id), C.c_int32(search_list_size), C.c_int32(compression_type),
                                                 pi, pmd, nmd, pmi, nmi, C.c_void_p(image.ctypes.data), C.c_int64(max(size, 0)),
                                                 C.byref(written), _stream_ptr(stream)))
        return image[:written.value].tobytes()

    def _graph_search(self, fn, queries, k, mid_arg, want_stats, stream):
        nq = _rows(queries, self.dim)
        q, pq_ = _ptr(queries, np.float32)
        ids = _empty_like(queries, (nq, k), np.uint32)
        scores = _empty_like(queries, (nq, k), np.float32)
        i, pi = _ptr(ids, np.uint32)
        s_, ps = _ptr(scores, np.float32)
        stats = np.zeros((nq, 5), np.int64) if want_stats else None
        pst = C.c_void_p(stats.ctypes.data) if want_stats else None
        check(fn(self._h, pq_, C.c_int64(nq), C.c_int32(k), C.c_int32(mid_arg), pi, ps, pst, _stream_ptr(stream)))
        if want_stats and want_stats != "full":
            stats = stats[:, :4]     # the reference's FilterGateStats columns; "full" adds descent_distance_computations
        return (ids, scores, stats) if want_stats else (ids, scores)

    def search_hnsw(self, queries, k, ef, stats=False, stream=None):
        """hnsw.KNNSearch (hnsw.go:1650-1755); stats columns: nodes_visited,
        distance_computations, distance_short_circuits, pops (stats="full": + rows scored by the descent)."""
        return self._graph_search(self._lib.vg_search_hnsw, queries, k, ef, stats, stream)

    def search_hnsw_pq(self, queries, k, ef, stats=False, stream=None):
        """searchLayer with distFunc = pq.ComputeAsymmetricDistance over the nodes' PQ codes (the candidate
        stage of graph -> PQ -> exact rerank); scores are PQ distances."""
        return self._graph_search(self._lib.vg_search_hnsw_pq, queries, k, ef, stats, stream)

    def _packed_mask(self, mask, nq, what):
        """bool[n] / bool[nq, n] / packed little-endian bits -> (keepalive, void*, stride in bytes; 0 = one mask).  A torch
        uint8 tensor (host or device) is taken as packed bits where it lies."""
        if _is_torch(mask):
            if mask.dtype != torch.uint8:
                raise TypeError(f"{what}: a torch mask holds packed bits (uint8), got {mask.dtype}")
            m = mask if mask.is_contiguous() else mask.contiguous()
            if m.shape[-1] < (self.n + 7) // 8:
                raise ValueError(f"{what}: a packed mask holds ceil(n / 8) = {(self.n + 7) // 8} bytes, got {m.shape[-1]}")
            stride = 0
            if m.ndim > 1 and m.shape[0] > 1:
                if m.shape[0] != nq:
                    raise ValueError(f"{what}: one mask per query ({nq}), got {m.shape[0]}")
                stride = m.shape[1]
            return m, C.c_void_p(m.data_ptr()), stride
        m = np.asarray(mask)
        if m.dtype == np.bool_:
            if m.shape[-1] != self.n:   # the C side reads ceil(n / 8) bytes per mask: a short one would be read past its end
                raise ValueError(f"{what}: a bool mask has one entry per row ({self.n}), got {m.shape[-1]}")
            m = np.packbits(m.reshape(-1, self.n) if m.ndim > 1 else m, axis=-1, bitorder="little")
        m = np.ascontiguousarray(m, np.uint8)
        if m.shape[-1] < (self.n + 7) // 8:
            raise ValueError(f"{what}: a packed mask holds ceil(n / 8) = {(self.n + 7) // 8} bytes, got {m.shape[-1]}")
        stride = 0
        if m.ndim > 1 and m.shape[0] > 1:
            if m.shape[0] != nq:
                raise ValueError(f"{what}: one mask per query ({nq}), got {m.shape[0]}")
            stride = m.shape[1]
        return m, C.c_void_p(m.ctypes.data), stride

    def search_hnsw_filtered(self, queries, k, ef, mask, selectivity, stats=False, stream=None):
        """searchExecute with a filter whose selectivity hint is above 0.3: searchLayerWithPostFilter (hnsw.go:1159-1218) —
        the walk with an expanded ef, the results re-filtered through `mask` (bool[n] / packed bits, one for the batch or
        one per query) and capped at ef.  `ef` = what determineEF returned."""
        nq = _rows(queries, self.dim)
        m, pm, stride = self._packed_mask(mask, nq, "search_hnsw_filtered")
        q, pq_ = _ptr(queries, np.float32)
        ids = _empty_like(queries, (nq, k), np.uint32)
        scores = _empty_like(queries, (nq, k), np.float32)
        i, pi = _ptr(ids, np.uint32)
        s_, ps = _ptr(scores, np.float32)
        st = np.zeros((nq, 5), np.int64) if stats else None
        pst = C.c_void_p(st.ctypes.data) if stats else None
        check(self._lib.vg_search_hnsw_filtered(self._h, pq_, C.c_int64(nq), C.c_int32(k), C.c_int32(ef), pm,
                                                C.c_int64(stride), C.c_double(float(selectivity)), pi, ps, pst, _stream_ptr(stream)))
        if stats and stats != "full":
            st = st[:, :4]
        return (ids, scores, st) if stats else (ids, scores)

    def set_hnsw_edge_distances(self, l0_dist=None, stream=None):
        """The layer-0 lists' cached Neighbor.Dist [n, m0] (node.go:62-80) for search_hnsw_predicate; None = recompute them
        from the fp32 rows (the distance between the two nodes, what the insert stored)."""
        if l0_dist is None:
            check(self._lib.vg_index_set_hnsw_edge_distances(self._h, None, _stream_ptr(stream)))
            return
        d, pd = _ptr(l0_dist, np.float32)
        check(self._lib.vg_index_set_hnsw_edge_distances(self._h, pd, _stream_ptr(stream)))

    def set_hnsw_tombstones(self, deleted=None, stream=None):
        """g.tombstones (hnsw.go:95): bool[n] / packed bits, None clears.  Deleted nodes are walked through, never returned
        (hnsw.go:1381-1390); read by search_hnsw, search_hnsw_pq, search_hnsw_filtered, search_hnsw_predicate."""
        if deleted is None:
            check(self._lib.vg_index_set_hnsw_tombstones(self._h, None, _stream_ptr(stream)))
            return
        d, pd, _ = self._packed_mask(deleted, 1, "set_hnsw_tombstones")
        check(self._lib.vg_index_set_hnsw_tombstones(self._h, pd, _stream_ptr(stream)))

    def search_hnsw_predicate(self, queries, k, ef, mask, deleted=None, stats=False, stream=None):
        """searchExecute with a filter whose selectivity hint is <= 0.3 or unknown: searchLayerPredicateAware
        (hnsw.go:1406-1558).  mask: filter.Matches (bool[n] / packed bits, one for the batch or one per query); deleted: the
        tombstone bitmap (bool[n] / packed bits) or None.  stats columns: nodes_visited, distance_computations,
        ExpansionsSkipped, pops."""
        nq = _rows(queries, self.dim)
        m, pm, stride = self._packed_mask(mask, nq, "search_hnsw_predicate")
        d, pdl, _ = (None, None, 0) if deleted is None else self._packed_mask(deleted, 1, "search_hnsw_predicate (deleted)")
        q, pq_ = _ptr(queries, np.float32)
        ids = _empty_like(queries, (nq, k), np.uint32)
        scores = _empty_like(queries, (nq, k), np.float32)
        i, pi = _ptr(ids, np.uint32)
        s_, ps = _ptr(scores, np.float32)
        st = np.zeros((nq, 5), np.int64) if stats else None
        pst = C.c_void_p(st.ctypes.data) if stats else None
        check(self._lib.vg_search_hnsw_predicate(self._h, pq_, C.c_int64(nq), C.c_int32(k), C.c_int32(ef), pm, C.c_int64(stride), pdl,
                                                 pi, ps, pst, _stream_ptr(stream)))
        if stats and stats != "full":
            st = st[:, :4]
        return (ids, scores, st) if stats else (ids, scores)

    BRUTE_SCAN, BRUTE_BITMAP = 0, 1

    def search_hnsw_brute(self, queries, k, mode=0, mask=None, stream=None):
        """hnsw.BruteSearch + scanSegment (hnsw.go:2021-2101; mode BRUTE_SCAN) or searchBitmap + extraction
        (:2240-2263, :1732-1751; BRUTE_BITMAP): every row whose mask bit is set, in id order, through the
        reference's PriorityQueue.  mask: None, bool[n] / packed bits for the whole batch, or bool[nq, n] / packed
        [nq, ceil(n/8)] for one mask per query.  HNSW distances (L2, -dot, 0.5 * L2), best first."""
        nq = _rows(queries, self.dim)
        q, pq_ = _ptr(queries, np.float32)
        ids = _empty_like(queries, (nq, k), np.uint32)
        scores = _empty_like(queries, (nq, k), np.float32)
        i, pi = _ptr(ids, np.uint32)
        s_, ps = _ptr(scores, np.float32)
        m, pm, stride = (None, None, 0) if mask is None else self._packed_mask(mask, nq, "search_hnsw_brute")
        check(self._lib.vg_search_hnsw_brute(self._h, pq_, C.c_int64(nq), C.c_int32(k), C.c_int32(mode), pm,
                                             C.c_int64(stride), pi, ps, _stream_ptr(stream)))
        return ids, scores

    def search_vamana(self, queries, k, kind=0, stats=False, stream=None):
        """diskann searchInternal (diskann/segment.go:503-706); kind 0 fp32, 1 PQ, 2 RaBitQ, 3 INT4."""
        return self._graph_search(self._lib.vg_search_vamana, queries, k, kind, stats, stream)

    def search_vamana_filtered(self, queries, k, mask, kind=0, stats=False, stream=None):
        """searchInternal with `filter` set (diskann/segment.go:616-627): rows whose mask entry is clear are walked through
        but never enter the result heap.  mask: bool[n] / packed bits for the batch, or one per query."""
        if mask is None:
            return self.search_vamana(queries, k, kind, stats, stream)
        nq = _rows(queries, self.dim)
        m, pm, stride = self._packed_mask(mask, nq, "search_vamana_filtered")
        q, pq_ = _ptr(queries, np.float32)
        ids = _empty_like(queries, (nq, k), np.uint32)
        scores = _empty_like(queries, (nq, k), np.float32)
        i, pi = _ptr(ids, np.uint32)
        s_, ps = _ptr(scores, np.float32)
        st = np.zeros((nq, 5), np.int64) if stats else None
        pst = C.c_void_p(st.ctypes.data) if stats else None
        check(self._lib.vg_search_vamana_filtered(self._h, pq_, C.c_int64(nq), C.c_int32(k), C.c_int32(kind), pm, C.c_int64(stride),
                                                  pi, ps, pst, _stream_ptr(stream)))
        if stats and stats != "full":
            st = st[:, :4]
        return (ids, scores, st) if stats else (ids, scores)

    def search_vamana_threshold(self, queries, thresholds, max_results, kind=0, mask=None, stats=False, stream=None):
        """Engine.SearchThreshold's DiskANN leg (engine/engine.go:1485-1531): search_vamana_filtered(q, max_results), then the rows
        with score <= threshold (L2) / >= threshold (Dot, Cosine) in walk order.  thresholds: a scalar for the batch or one per
        query; mask: as search_vamana_filtered's (None = no filter).  Returns (ids [nq, max_results], scores, counts [nq]) and
        the stats with stats=True: query q's rows are ids[q, :counts[q]], the rest padded with 0xFFFFFFFF / +-Inf."""
        nq = _rows(queries, self.dim)
        q, pq_ = _ptr(queries, np.float32)
        if _is_torch(thresholds):
            t = thresholds.to(torch.float32).reshape(-1)
            if t.numel() == 1 and nq != 1:
                t = t.expand(nq)
            t = t.contiguous()
        else:
            t = np.asarray(thresholds, np.float32).reshape(-1)
            if t.size == 1:
                t = np.full(nq, t[0], np.float32)
        if (t.numel() if _is_torch(t) else t.size) != nq:
            raise ValueError(f"search_vamana_threshold: one threshold for the batch or one per query ({nq})")
        t, pt = _ptr(t, np.float32, nq)
        m, pm, stride = (None, None, 0) if mask is None else self._packed_mask(mask, nq, "search_vamana_threshold")
        ids = _empty_like(queries, (nq, max_results), np.uint32)
        scores = _empty_like(queries, (nq, max_results), np.float32)
        counts = _empty_like(queries, (nq,), np.int32)
        i, pi = _ptr(ids, np.uint32, nq * max_results)
        s, ps = _ptr(scores, np.float32, nq * max_results)
        c, pc = _ptr(counts, np.int32, nq)
        st = np.zeros((nq, 5), np.int64) if stats else None
        pst = C.c_void_p(st.ctypes.data) if stats and nq else None
        check(self._lib.vg_search_vamana_threshold(self._h, pq_, C.c_int64(nq), pt, C.c_int32(max_results), C.c_int32(kind), pm,
                                                   C.c_int64(stride), pi, ps, pc, pst, _stream_ptr(stream)))
        if not stats:
            return ids, scores, counts
        return ids, scores, counts, (st if stats == "full" else st[:, :4])

    def set_vectors(self, base, stream=None):
        """fp32 rows, n*dim row-major (vectorstore/columnar.go:21-24)."""
        b, pb = _ptr(base, np.float32, self.n * self.dim)
        check(self._lib.vg_index_set_vectors(self._h, pb, _stream_ptr(stream)))

    def rerank(self, queries, cand_ids, k, out=None, stream=None):
        """Segment.Rerank + top-k (flat/segment.go:754-780): cand_ids is [nq, nc]."""
        nq = _rows(queries, self.dim)
        nc = (cand_ids.numel() if _is_torch(cand_ids) else np.asarray(cand_ids).size) // max(nq, 1)
        q, pq_ = _ptr(queries, np.float32)
        c, pc = _ptr(cand_ids, np.uint32, nq * nc)
        if out is None:
            out = (_empty_like(queries, (nq, k), np.uint32), _empty_like(queries, (nq, k), np.float32))
        i, pi = _ptr(out[0], np.uint32, nq * k)
        s, ps = _ptr(out[1], np.float32, nq * k)
        check(self._lib.vg_rerank(self._h, pq_, C.c_int64(nq), pc, C.c_int32(nc), C.c_int32(k), pi, ps,
                                  _stream_ptr(stream)))
        return out

    def robust_prune(self, nodes, cands, r, alpha=1.2, stream=None):
        """Vamana robustPrune (diskann/writer.go:571-625) for a batch of nodes: cands is [n_nodes, nc]
        uint32 (VG_INVALID_ID padded); returns (kept[n_nodes, r], counts[n_nodes])."""
        nd = np.ascontiguousarray(nodes, np.uint32)
        cd = np.ascontiguousarray(cands, np.uint32).reshape(nd.size, -1)
        out = np.empty((nd.size, r), np.uint32); cnt = np.empty(nd.size, np.int32)
        check(self._lib.vg_robust_prune(self._h, C.c_void_p(nd.ctypes.data), C.c_int64(nd.size),
                                        C.c_void_p(cd.ctypes.data), C.c_int32(cd.shape[1]), C.c_int32(r),
                                        C.c_float(alpha), C.c_void_p(out.ctypes.data), C.c_void_p(cnt.ctypes.data),
                                        _stream_ptr(stream)))
        return out, cnt

    def hnsw_select_neighbors(self, cand_ids, cand_dists, m, stream=None):
        """HNSW selectNeighborsHeuristic (hnsw.go:1009-1106) for a batch of nodes: cand_ids / cand_dists
        are [n_nodes, nc], nearest first; returns (kept[n_nodes, m], counts[n_nodes])."""
        ci = np.ascontiguousarray(cand_ids, np.uint32)
        cdst = np.ascontiguousarray(cand_dists, np.float32)
        nn, nc = ci.shape
        out = np.empty((nn, m), np.uint32); cnt = np.empty(nn, np.int32)
        check(self._lib.vg_hnsw_select_neighbors(self._h, C.c_int64(nn), C.c_void_p(ci.ctypes.data),
                                                 C.c_void_p(cdst.ctypes.data), C.c_int32(nc), C.c_int32(m),
                                                 C.c_void_p(out.ctypes.data), C.c_void_p(cnt.ctypes.data),
                                                 _stream_ptr(stream)))
        return out, cnt

    def score_candidates(self, queries, cand_ids, out=None, stream=None):
        nq = _rows(queries, self.dim)
        nc = (cand_ids.numel() if _is_torch(cand_ids) else np.asarray(cand_ids).size) // max(nq, 1)
        q, pq_ = _ptr(queries, np.float32)
        c, pc = _ptr(cand_ids, np.uint32, nq * nc)
        if out is None:
            out = _empty_like(queries, (nq, nc), np.float32)
        s, ps = _ptr(out, np.float32, nq * nc)
        check(self._lib.vg_score_candidates(self._h, pq_, C.c_int64(nq), pc, C.c_int32(nc), ps,
                                            _stream_ptr(stream)))
        return out

    def _search(self, fn, queries, k, extra=(), out=None, stream=None):
        nq = _rows(queries, self.dim)
        q, pq_ = _ptr(queries, np.float32)
        if out is None:
            ids = _empty_like(queries, (nq, k), np.uint32)
            scores = _empty_like(queries, (nq, k), np.float32)
        else:
            ids, scores = out
        i, pi = _ptr(ids, np.uint32, nq * k)
        s, ps = _ptr(scores, np.float32, nq * k)
        check(fn(self._h, pq_, C.c_int64(nq), C.c_int32(k), *extra, pi, ps, _stream_ptr(stream)))
        return ids, scores

    def search_flat(self, queries, k, out=None, stream=None):
        """flat.Segment.Search fp32 branch / hnsw.BruteSearch: exact brute force."""
        return self._search(self._lib.vg_search_flat, queries, k, out=out, stream=stream)

    def _threshold_search(self, name, call, queries, thresholds, max_results, mask, out):
        """The operands every threshold search shares, staged; call(queries, nq, thresholds, mask, mask_stride, ids, scores,
        counts) is the entry point with them."""
        nq = _rows(queries, self.dim)
        q, pq_ = _ptr(queries, np.float32)
        if _is_torch(thresholds):
            t = thresholds.to(torch.float32).reshape(-1)
            if t.numel() == 1 and nq != 1:
                t = t.expand(nq)
            t = t.contiguous()
        else:
            t = np.asarray(thresholds, np.float32).reshape(-1)
            if t.size == 1:
                t = np.full(nq, t[0], np.float32)
        if (t.numel() if _is_torch(t) else t.size) != nq:
            raise ValueError(f"{name}: one threshold for the batch or one per query ({nq})")
        t, pt = _ptr(t, np.float32, nq)
        m, pm, stride = (None, None, 0) if mask is None else self._packed_mask(mask, nq, name)
        if out is None:
            ids = _empty_like(queries, (nq, max_results), np.uint32)
            scores = _empty_like(queries, (nq, max_results), np.float32)
            counts = _empty_like(queries, (nq,), np.int32)
        else:
            ids, scores, counts = out
        i, pi = _ptr(ids, np.uint32, nq * max_results)
        s, ps = _ptr(scores, np.float32, nq * max_results)
        c, pc = _ptr(counts, np.int32, nq)
        check(call(pq_, C.c_int64(nq), pt, pm, C.c_int64(stride), pi, ps, pc))
        return ids, scores, counts

    def search_flat_threshold(self, queries, thresholds, max_results, mask=None, out=None, stream=None):
        """Engine.SearchThreshold over this flat segment (engine/engine.go:1485-1531): search_flat(q, max_results), then the rows
        with score <= threshold (L2) / >= threshold (Dot, Cosine), best first.  thresholds: a scalar for the batch or one per
        query; mask: as search_flat_filtered's (None = no filter).  Returns (ids [nq, max_results], scores, counts [nq]): query
        q's rows are ids[q, :counts[q]], the rest padded with 0xFFFFFFFF / +-Inf."""
        def call(pq_, nq, pt, pm, stride, pi, ps, pc):
            return self._lib.vg_search_flat_threshold(self._h, pq_, nq, pt, C.c_int32(max_results), pm, stride, pi, ps, pc,
                                                      _stream_ptr(stream))
        return self._threshold_search("search_flat_threshold", call, queries, thresholds, max_results, mask, out)

    def search_flat_probed_threshold(self, queries, thresholds, max_results, nprobes=0, scan=0, rerank=False, mask=None, out=None,
                                     stream=None):
        """Engine.SearchThreshold over a flat segment with codes and / or IVF partitions (engine/engine.go:1485-1531 over
        flat/segment.go:447-780): the best max_results rows of the probed partitions (or the whole segment) by the score of
        `scan` (SCAN_F32 / SCAN_PQ / SCAN_SQ8), then the rows within the threshold, best first.  rerank=False compares the
        threshold with the scan score (the segment-level answer); rerank=True re-scores the candidates exactly from the fp32
        rows first and compares that (the engine's).  Operands and result as search_flat_threshold's."""
        def call(pq_, nq, pt, pm, stride, pi, ps, pc):
            return self._lib.vg_search_flat_probed_threshold(self._h, pq_, nq, pt, C.c_int32(max_results), C.c_int32(nprobes),
                                                             C.c_int32(scan), C.c_int32(1 if rerank else 0), pm, stride, pi, ps, pc,
                                                             _stream_ptr(stream))
        return self._threshold_search("search_flat_probed_threshold", call, queries, thresholds, max_results, mask, out)

    def enable_bf16_filter(self, on: bool = True, stream=None):
        """vg_index_enable_bf16_filter: nominate with a bfloat16 MFMA GEMM over a bf16 copy of the rows; the exact fp32
        re-score and the (widened) proof keep ids and scores bit-identical."""
        check(self._lib.vg_index_enable_bf16_filter(self._h, C.c_int32(1 if on else 0), _stream_ptr(stream)))

    def flat_stats(self, stream=None):
        """(queries searched, queries answered by the exhaustive kernel) since set_vectors."""
        q, e = C.c_int64(0), C.c_int64(0)
        check(self._lib.vg_index_flat_stats(self._h, C.byref(q), C.byref(e), _stream_ptr(stream)))
        return q.value, e.value

    def flat_retried(self, stream=None):
        """vg_index_flat_retried: queries of search_flat since set_vectors that the one-product screen could not prove and the
        three-product pass nominated again."""
        r = C.c_int64(0)
        check(self._lib.vg_index_flat_retried(self._h, C.byref(r), _stream_ptr(stream)))
        return r.value

    def flat_appended(self, stream=None):
        """vg_index_flat_appended: the candidates search_flat's nomination appended to its queries' lists since set_vectors, summed
        over the queries of the GEMM path (long lists: thresholds too high; too low shows in flat_stats()[1])."""
        r = C.c_int64(0)
        check(self._lib.vg_index_flat_appended(self._h, C.byref(r), _stream_ptr(stream)))
        return r.value

    def search_pq_adc(self, queries, k, out=None, stream=None):
        """flat.Segment.Search PQ branch (flat/segment.go:476-483,678-689,714-721)."""
        return self._search(self._lib.vg_search_pq_adc, queries, k, out=out, stream=stream)


INVALID_ID = 0xFFFFFFFF   # VG_INVALID_ID


def merge_indexes(ctx: Context, sources, deleted=None, stream=None):
    """Engine.CompactWithContext's Iterate loop (engine/compaction.go:173-218) over resident indexes (vg_index_merge; the
    rules are the header's): the live rows of sources[0], then of sources[1], ..., in row order, as a new Index.  deleted:
    None, or one entry per source, each None / bool[n_s] / packed bits (numpy, or a torch uint8 tensor where it lies).
    Returns (index, old_to_new, new_source, new_row): old_to_new is np.uint32 over the concatenated source rows (INVALID_ID =
    deleted), new_source np.int32 and new_row np.uint32 have one entry per row of the new index."""
    sources = list(sources)
    if deleted is not None and len(deleted) != len(sources):
        raise ValueError(f"merge_indexes: one deleted entry per source ({len(sources)}), got {len(deleted)}")
    keep, ptrs = [], []
    for s, src in enumerate(sources):
        d = None if deleted is None else deleted[s]
        if d is None or src.n == 0:
            ptrs.append(None)
            continue
        m, pm, _ = src._packed_mask(d, 1, "merge_indexes")
        keep.append(m)
        ptrs.append(pm.value)
    handles = (C.c_void_p * len(sources))(*[src._h.value for src in sources])
    bitmaps = (C.c_void_p * len(sources))(*ptrs)
    total = sum(src.n for src in sources)
    old_to_new = np.empty(total, np.uint32)
    new_source = np.empty(total, np.int32)
    new_row = np.empty(total, np.uint32)
    out = C.c_void_p()
    check(ctx._lib.vg_index_merge(ctx._h, handles, None if deleted is None else bitmaps, C.c_int32(len(sources)), C.byref(out),
                                  C.c_void_p(old_to_new.ctypes.data), C.c_void_p(new_source.ctypes.data),
                                  C.c_void_p(new_row.ctypes.data), _stream_ptr(stream)))
    live = int(np.count_nonzero(old_to_new != INVALID_ID))
    merged = Index._adopted(ctx, out, live, sources[0].dim, int(sources[0].metric))
    return merged, old_to_new, new_source[:live].copy(), new_row[:live].copy()


def compaction_plan(total_rows: int, diskann_threshold: int = 0):
    """The writer Engine.CompactWithContext chooses (engine/compaction.go:86-152) for `total_rows` source rows, deleted ones
    included (it sums RowCount() before it looks at tombstones): ("diskann", 0) from diskann_threshold rows up (0 or less:
    10000), else ("flat", k) with k = max(1, total_rows // 8192) partitions."""
    threshold = diskann_threshold if diskann_threshold > 0 else 10000
    if total_rows >= threshold:
        return "diskann", 0
    return "flat", max(1, total_rows // 8192)


def compact(ctx: Context, sources, deleted=None, *, diskann_threshold=0, flat_quantizer=None, diskann=None, seed=0, stream=None):
    """Engine.CompactWithContext on resident indexes: compaction_plan over the sources' row counts, merge_indexes, then the
    chosen writer on the result — Index.flat_build(k, flat_quantizer, seed) or Index.diskann_build(seed=seed, **diskann)
    (diskann: a dict of diskann_build's r / l / alpha / quantizer / pq_iters / max_batch / growth_div; unset ones take
    diskann.DefaultOptions: 64 / 100 / 1.2 / no codes).  What the builders do with few rows passes through: flat_build leaves
    fewer live rows than k unpartitioned, diskann_build refuses 0 rows ("no vectors to write").
    Returns (index, kind, old_to_new, new_source, new_row) with the FINAL positions: merge_indexes' maps composed with the
    builder's perm / inv_perm (the reference's flat NewRowID is right only for k = 1, compaction.go:205-206; these are the
    rows' true places).  Ids, metadata and payloads are the caller's to move with new_source / new_row."""
    sources = list(sources)
    kind, k = compaction_plan(sum(src.n for src in sources), diskann_threshold)
    merged, old_to_new, new_source, new_row = merge_indexes(ctx, sources, deleted, stream=stream)
    try:
        if kind == "flat":
            perm, inv = merged.flat_build(k, quantizer=flat_quantizer, seed=seed, stream=stream)
        else:
            perm, inv, _ = merged.diskann_build(seed=seed, stream=stream, **(diskann or {}))
    except Exception:
        merged.close()
        raise
    live = old_to_new != INVALID_ID
    final = old_to_new.copy()
    final[live] = inv[old_to_new[live]]
    return merged, kind, final, new_source[perm], new_row[perm]


class SegmentInfo(C.Structure):
    _fields_ = [("segment_id", C.c_uint64), ("rows", C.c_int64), ("dim", C.c_int32), ("metric", C.c_int32),
                ("kind", C.c_int32), ("quantization", C.c_int32), ("pq_m", C.c_int32), ("pq_k", C.c_int32),
                ("max_degree", C.c_int32), ("search_list_size", C.c_int32), ("entrypoint", C.c_uint32),
                ("num_partitions", C.c_int32)]


class Segment:
    """A flat or DiskANN segment file of the reference (internal/segment/flat/format.go,
    internal/segment/diskann/format.go) opened straight onto the GPU: `image` is the whole file
    as bytes / numpy uint8 / np.memmap.  `index` is searched like any other Index."""

    def __init__(self, ctx: Context, image, kind: str = "flat", verify_checksum: bool = True, stream=None):
        self._lib, self.ctx = ctx._lib, ctx
        buf = np.frombuffer(image, np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(image, np.uint8)
        fn = {"flat": self._lib.vg_segment_open_flat, "diskann": self._lib.vg_segment_open_diskann}[kind]
        h = C.c_void_p()
        check(fn(ctx._h, C.c_void_p(buf.ctypes.data), C.c_int64(buf.size), C.c_int32(int(verify_checksum)),
                 C.byref(h), _stream_ptr(stream)))
        self._h = h
        info = SegmentInfo()
        check(self._lib.vg_segment_get_info(self._h, C.byref(info)))
        self.info = info
        self._lib.vg_segment_index.restype = C.c_void_p
        ih = C.c_void_p(self._lib.vg_segment_index(self._h))
        self.index = Index._borrowed(ctx, ih, int(info.rows), int(info.dim), int(info.metric), self)

    def search(self, queries, k, nprobes=0, out=None, stream=None):
        """flat.Segment.Search (flat/segment.go:447-751): scan type by the segment's quantization,
        IVF partitions probed when the segment has more than one."""
        seg = self._h

        def fn(_index_handle, *args):  # same argument list as the index searches, segment handle first
            return self._lib.vg_segment_search(seg, *args)
        return self.index._search(fn, queries, k, extra=(C.c_int32(nprobes),), out=out, stream=stream)

    def search_filtered(self, queries, k, mask, nprobes=0, out=None, stream=None):
        """Segment.Search with a row filter (flat/segment.go:631-635, diskann/segment.go:616-627): mask bool[n] / packed bits
        for the batch or one per query; None = search."""
        if mask is None:
            return self.search(queries, k, nprobes, out=out, stream=stream)
        seg = self._h
        m, pm, stride = self.index._packed_mask(mask, _rows(queries, self.index.dim), "Segment.search_filtered")

        def fn(_index_handle, *args):
            return self._lib.vg_segment_search_filtered(seg, *args)
        return self.index._search(fn, queries, k, extra=(C.c_int32(nprobes), pm, C.c_int64(stride)), out=out, stream=stream)

    def search_threshold(self, queries, thresholds, max_results, nprobes=0, rerank=False, mask=None, out=None, stream=None):
        """Engine.SearchThreshold over this segment, by what the file holds: search_flat_probed_threshold with the segment's
        scan on a flat segment, search_vamana_threshold with its kind on a DiskANN one (nprobes and rerank unused there)."""
        seg = self._h

        def call(pq_, nq, pt, pm, stride, pi, ps, pc):
            return self._lib.vg_segment_search_threshold(seg, pq_, nq, pt, C.c_int32(max_results), C.c_int32(nprobes),
                                                         C.c_int32(1 if rerank else 0), pm, stride, pi, ps, pc, _stream_ptr(stream))
        return self.index._threshold_search("Segment.search_threshold", call, queries, thresholds, max_results, mask, out)

    def close(self):
        if getattr(self, "_h", None):
            self.index._h = None
            self._lib.vg_segment_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def crc32c(data) -> int:
    """hash.CRC32C (internal/hash/crc32c.go:15-17) as computed by the library."""
    from . import _lib
    lib = _lib.load()
    lib.vg_crc32c.restype = C.c_uint32
    buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(data, np.uint8)
    return int(lib.vg_crc32c(C.c_void_p(buf.ctypes.data), C.c_int64(buf.size)))


def crc32c_device(ctx: Context, data, stream=None) -> int:
    """hash.CRC32C of a device buffer (a torch tensor on the GPU, any dtype, contiguous), computed there: vg_crc32c_device."""
    if not _is_torch(data) or not data.is_cuda:
        raise TypeError("crc32c_device takes a torch tensor in device memory (crc32c is the host's)")
    if not data.is_contiguous():
        raise ValueError("crc32c_device: the tensor must be contiguous")
    out = C.c_uint32(0)
    check(ctx._lib.vg_crc32c_device(ctx._h, C.c_void_p(data.data_ptr()), C.c_int64(data.numel() * data.element_size()), C.byref(out),
                                    _stream_ptr(stream)))
    return int(out.value)


# ---- metadata filters on the device (vg_columns_*, vg_filter_evaluate, vg_mask_*) ------------------------------------------
FILTER_TILE_ROWS = 4096   # VG_FILTER_TILE_ROWS: the rows one workgroup of vg_filter_evaluate owns (the tests' row seams)
MASK_ROWS_TILE_ROWS = 8192    # VG_MASK_ROWS_TILE_ROWS: the rows one workgroup of mask_to_rows compacts (the tests' row seams)
PREFILTER_CHUNK_ROWS = 256    # VG_PREFILTER_CHUNK_ROWS: the listed rows one workgroup of search_flat_prefilter scores


class FilterOp(enum.IntEnum):
    """metadata.Operator as vg_filter_clause.op (VG_FILTER_*)."""
    EQ = 0
    NE = 1
    LT = 2
    LTE = 3
    GT = 4
    GTE = 5
    IN = 6


class MaskOp(enum.IntEnum):
    """VG_MASK_*: simd.AndWords / AndNotWords / OrWords / XorWords (internal/simd/bitmap.go:26-48)."""
    AND = 0
    ANDNOT = 1
    OR = 2
    XOR = 3


# vg_filter_clause: 32 bytes, `reserved` 0
FILTER_CLAUSE = np.dtype({"names": ["field", "op", "value", "code", "set_begin", "set_count", "reserved"],
                          "formats": [np.int32, np.int32, np.float64, np.uint32, np.int32, np.int32, np.int32],
                          "offsets": [0, 4, 8, 16, 20, 24, 28], "itemsize": 32})


def pack_filter_sets(filter_sets):
    """[[(field, op, value-or-codes), ...] per query] -> (clauses: FILTER_CLAUSE[total], clause_off: int32[nq + 1],
    sets: uint32[n_sets]) as vg_filter_evaluate reads them.  op: a FilterOp, its number or its name ("eq" ... "in").  An
    `in` filter's third entry is its codes, appended to `sets`.  Any other filter's third entry goes into BOTH operand
    fields, since which one is read depends on the column behind the field: `value` = float(v), and `code` = v where v is
    an integer in uint32 range (INVALID_ID otherwise: no row holds it)."""
    clauses, off, sets = [], [0], []
    for fs in filter_sets:
        for field, op, operand in fs:
            op = FilterOp[op.upper()] if isinstance(op, str) else FilterOp(int(op))
            rec = np.zeros((), FILTER_CLAUSE)
            rec["field"], rec["op"] = int(field), int(op)
            if op == FilterOp.IN:
                codes = np.asarray(operand, np.uint32).reshape(-1)
                rec["set_begin"], rec["set_count"] = len(sets), codes.size
                rec["code"] = INVALID_ID
                sets.extend(codes.tolist())
            else:
                rec["value"] = float(operand)
                integral = isinstance(operand, (int, np.integer)) and not isinstance(operand, bool) and 0 <= int(operand) <= INVALID_ID
                rec["code"] = int(operand) if integral else INVALID_ID
            clauses.append(rec)
        off.append(len(clauses))
    packed = np.array(clauses, FILTER_CLAUSE) if clauses else np.zeros(0, FILTER_CLAUSE)
    return packed, np.asarray(off, np.int32), np.asarray(sets, np.uint32)


def _packed_bits(x, rows, what):
    """bool[rows] / packed little-endian bits (numpy uint8, or a torch uint8 tensor where it lies) -> (keepalive, void*)"""
    if x is None:
        return None, None
    if _is_torch(x):
        if x.dtype != torch.uint8:
            raise TypeError(f"{what}: a torch bitmap holds packed bits (uint8), got {x.dtype}")
        m = x if x.is_contiguous() else x.contiguous()
        if m.numel() < (rows + 7) // 8:
            raise ValueError(f"{what}: a packed bitmap holds ceil(rows / 8) = {(rows + 7) // 8} bytes, got {m.numel()}")
        return m, C.c_void_p(m.data_ptr())
    m = np.asarray(x)
    if m.dtype == np.bool_:
        if m.size != rows:
            raise ValueError(f"{what}: a bool bitmap has one entry per row ({rows}), got {m.size}")
        m = np.packbits(m.reshape(-1), bitorder="little")
    m = np.ascontiguousarray(m, np.uint8)
    if m.size < (rows + 7) // 8:
        raise ValueError(f"{what}: a packed bitmap holds ceil(rows / 8) = {(rows + 7) // 8} bytes, got {m.size}")
    return m, C.c_void_p(m.ctypes.data)


class Columns:
    """The resident metadata columns of one segment (vg_columns): per field 0..63 one f64 per row with a presence bitmap
    (numeric fields) or one uint32 dictionary code per row (categorical fields; INVALID_ID = no value)."""

    def __init__(self, ctx: Context, rows: int):
        self._lib = ctx._lib
        self._ctx = ctx
        h = C.c_void_p()
        check(self._lib.vg_columns_create(ctx._h, C.c_int64(rows), C.byref(h)))
        self._h = h
        self.rows = rows

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vg_columns_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_f64(self, field: int, values, present=None, stream=None):
        """values: float64[rows] (numpy, or a torch float64 tensor where it lies); present: bool[rows] / packed bits, None =
        every row has a value.  Replaces whatever the field held."""
        if _is_torch(values):
            if values.dtype != torch.float64 or values.numel() != self.rows:
                raise TypeError(f"set_f64: a float64 tensor of {self.rows} values, got {values.dtype} x {values.numel()}")
            v = values.contiguous()
            pv = C.c_void_p(v.data_ptr())
        else:
            v = np.ascontiguousarray(values, np.float64)
            if v.size != self.rows:
                raise ValueError(f"set_f64: one value per row ({self.rows}), got {v.size}")
            pv = C.c_void_p(v.ctypes.data)
        p, pp = _packed_bits(present, self.rows, "set_f64 (present)")
        check(self._lib.vg_columns_set_f64(self._h, C.c_int32(field), pv, pp, _stream_ptr(stream)))

    def set_codes(self, field: int, codes, stream=None):
        """codes: uint32[rows] (numpy, or a torch int32 tensor where it lies), INVALID_ID = the row has no value."""
        c, pc = _ptr(codes, np.uint32)
        n = c.numel() if _is_torch(c) else c.size
        if n != self.rows:
            raise ValueError(f"set_codes: one code per row ({self.rows}), got {n}")
        check(self._lib.vg_columns_set_codes(self._h, C.c_int32(field), pc, _stream_ptr(stream)))

    def drop(self, field: int):
        check(self._lib.vg_columns_drop(self._h, C.c_int32(field)))


def _mask_batch(x, rows, what, writable=False):
    """a batch of packed masks where it lies: uint8 [nq, stride >= ceil(rows / 8)] or [ceil(rows / 8)] (one mask), numpy or
    torch, rows contiguous -> (keepalive, void*, nq, stride in bytes; 0 for a single 1-D mask)"""
    nbytes = (rows + 7) // 8
    if _is_torch(x):
        if x.dtype != torch.uint8 or x.ndim not in (1, 2) or (x.numel() and x.stride(-1) != 1):
            raise TypeError(f"{what}: packed masks are uint8 [nq, bytes] with contiguous rows")
        shape, stride, ptr = tuple(x.shape), (x.stride(0) if x.ndim == 2 else 0), x.data_ptr()
    else:
        if not isinstance(x, np.ndarray) or x.dtype != np.uint8 or x.ndim not in (1, 2) or (x.size and x.strides[-1] != 1):
            raise TypeError(f"{what}: packed masks are uint8 [nq, bytes] with contiguous rows")
        if writable and not x.flags.writeable:
            raise ValueError(f"{what}: the array is read-only")
        shape, stride, ptr = x.shape, (x.strides[0] if x.ndim == 2 else 0), x.ctypes.data
    if shape[-1] < nbytes:
        raise ValueError(f"{what}: a mask holds ceil(rows / 8) = {nbytes} bytes, got {shape[-1]}")
    return x, C.c_void_p(ptr), (shape[0] if len(shape) == 2 else 1), stride


def evaluate_filters(cols: Columns, filter_sets, deleted=None, out=None, counts=True, stream=None):
    """UnifiedIndex.EvaluateFilter (internal/metadata/unified.go:279-416) for a batch on the device (vg_filter_evaluate; the
    semantics are the header's).  filter_sets: one list of (field, op, value-or-codes) per query (pack_filter_sets); deleted:
    None / bool[rows] / packed bits, cleared from every mask.  out: None = a new torch uint8 tensor [nq, stride] on the
    context's device (stride = ceil(rows / 8) rounded up to 8 bytes; pass it with mask.stride(0) to the filtered searches, or
    as it is to Index.search_*_filtered), or a torch tensor / numpy array [nq, stride] to fill where it lies.
    Returns (masks, counts): counts int64[nq] on the masks' side (torch or numpy), None with counts=False."""
    clauses, off, sets = pack_filter_sets(filter_sets)
    nq = off.size - 1
    nbytes = (cols.rows + 7) // 8
    if out is None:
        if torch is None:
            raise RuntimeError("evaluate_filters: out=None makes a torch tensor; pass a numpy array without torch")
        out = torch.zeros((nq, (nbytes + 7) // 8 * 8), dtype=torch.uint8, device=f"cuda:{cols._ctx.device}")
    m, pm, mq, stride = _mask_batch(out, cols.rows, "evaluate_filters (out)", writable=True)
    if mq != nq:
        raise ValueError(f"evaluate_filters: one mask per query ({nq}), out has {mq}")
    cnt = pc = None
    if counts:
        cnt = torch.zeros(nq, dtype=torch.int64, device=out.device) if _is_torch(out) else np.zeros(nq, np.int64)
        pc = C.c_void_p(cnt.data_ptr() if _is_torch(cnt) else cnt.ctypes.data)
    d, pd = _packed_bits(deleted, cols.rows, "evaluate_filters (deleted)")
    check(cols._lib.vg_filter_evaluate(cols._h, C.c_void_p(clauses.ctypes.data) if clauses.size else None, C.c_void_p(off.ctypes.data),
                                       C.c_int64(nq), C.c_void_p(sets.ctypes.data) if sets.size else None, C.c_int64(sets.size), pd, pm,
                                       C.c_int64(stride), pc, _stream_ptr(stream)))
    return out, cnt


def mask_combine(ctx: Context, op, dst, src, rows: int, stream=None):
    """dst[q] = dst[q] OP src[q] in place over packed masks (vg_mask_combine; simd/bitmap.go:26-48).  dst: uint8 [nq, stride]
    or one 1-D mask; src: the same shape, or one 1-D mask for every query (a host-made mask, a tombstone bitmap).  numpy
    or torch, each on its own."""
    op = MaskOp[op.upper()] if isinstance(op, str) else MaskOp(int(op))
    d, pd, nq, dstride = _mask_batch(dst, rows, "mask_combine (dst)", writable=True)
    s, ps, sq, sstride = _mask_batch(src, rows, "mask_combine (src)")
    if sq != nq and not (sq == 1 and sstride == 0):
        raise ValueError(f"mask_combine: src holds {sq} masks, dst {nq}")
    if nq > 1 and dstride == 0:
        dstride = (rows + 7) // 8
    check(ctx._lib.vg_mask_combine(ctx._h, C.c_int32(int(op)), pd, C.c_int64(dstride), ps, C.c_int64(sstride if sq == nq and nq > 1 else 0),
                                   C.c_int64(nq), C.c_int64(rows), _stream_ptr(stream)))
    return dst


def mask_popcount(ctx: Context, mask, rows: int, stream=None):
    """int64[nq]: the set bits below `rows` of each packed mask (vg_mask_popcount; simd/bitmap.go:50-55), on the masks' side."""
    m, pm, nq, stride = _mask_batch(mask, rows, "mask_popcount")
    cnt = torch.zeros(nq, dtype=torch.int64, device=mask.device) if _is_torch(mask) else np.zeros(nq, np.int64)
    pc = C.c_void_p(cnt.data_ptr() if _is_torch(cnt) else cnt.ctypes.data)
    check(ctx._lib.vg_mask_popcount(ctx._h, pm, C.c_int64(stride), C.c_int64(nq), C.c_int64(rows), pc, _stream_ptr(stream)))
    return cnt


def mask_to_rows(ctx: Context, mask, rows: int, out_stride=None, out=None, counts=True, stream=None):
    """FilterResult.ToArrayInto for a batch of packed masks (vg_mask_to_rows; engine/search.go:617-627): per mask the ids of
    its set bits below `rows`, ascending, at most out_stride of them, the rest of its out_stride slots INVALID_ID — the
    block feeds Index.rerank / score_candidates as it is.  mask: uint8 [nq, stride] or one 1-D mask, numpy or torch, where it
    lies.  out: None = a new uint32 array [nq, out_stride] on the masks' side (torch: int32), or one to fill.  out_stride
    None = out's, or the largest count (which costs a count first); 0 = count only.  Returns (ids, counts): counts int64[nq] =
    ALL set bits of each mask, also past out_stride; None with counts=False."""
    m, pm, nq, stride = _mask_batch(mask, rows, "mask_to_rows")
    on_torch = _is_torch(mask)
    if out is not None:
        if out.ndim != 2 or out.shape[0] != nq:
            raise ValueError(f"mask_to_rows: out is [nq = {nq}, out_stride], got {tuple(out.shape)}")
        if out_stride is None:
            out_stride = out.shape[1]
        elif out_stride != out.shape[1]:
            raise ValueError(f"mask_to_rows: out has {out.shape[1]} slots per mask, out_stride is {out_stride}")
    elif out_stride is None:
        c = mask_popcount(ctx, mask, rows, stream=stream)
        out_stride = int(c.max()) if nq else 0
    cnt = pc = None
    if counts:
        cnt = torch.zeros(nq, dtype=torch.int64, device=mask.device) if on_torch else np.zeros(nq, np.int64)
        pc = C.c_void_p(cnt.data_ptr() if on_torch else cnt.ctypes.data)
    if out is None:
        out = torch.empty((nq, out_stride), dtype=torch.int32, device=mask.device) if on_torch else np.empty((nq, out_stride), np.uint32)
    o, po = _ptr(out, np.uint32, nq * out_stride)
    if o is not out:
        raise ValueError("mask_to_rows: out must be contiguous")
    check(ctx._lib.vg_mask_to_rows(ctx._h, pm, C.c_int64(stride), C.c_int64(nq), C.c_int64(rows), po if nq * out_stride else None,
                                   C.c_int64(out_stride), pc, _stream_ptr(stream)))
    return out, cnt


# ---- hybrid search: the resident BM25 index and Reciprocal Rank Fusion (vg_bm25_*, vg_rrf_fuse) ------------------------------
BM25_TILE_DOCS = 8192   # VG_BM25_TILE_DOCS: the docs one workgroup of Bm25.search scores (the tests' doc seams)
BM25_UPDATE_CHUNK = 2048   # VG_BM25_UPDATE_CHUNK: the postings one workgroup of Bm25.update's passes owns (the tests' posting seams)


def _ptr_f64(x, count):
    """(keepalive, void*) of float64 values: numpy, or a torch float64 tensor where it lies"""
    if _is_torch(x):
        if x.dtype != torch.float64:
            raise TypeError(f"expected torch.float64, got {x.dtype}")
        x = x if x.is_contiguous() else x.contiguous()
        n, p = x.numel(), x.data_ptr()
    else:
        x = np.ascontiguousarray(x, np.float64)
        n, p = x.size, x.ctypes.data
    if n < count:
        raise ValueError(f"buffer has {n} elements, need {count}")
    return x, C.c_void_p(p)


def _result_buffers(out, nq, k, like, device, counts=True):
    """ids uint32 / scores float32 [nq, k] and counts int32 [nq] (numpy, or torch on `device` when `like` is a torch tensor)"""
    if out is not None:
        return out
    if _is_torch(like):
        dev = like.device if like.is_cuda else f"cuda:{device}"
        return (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                torch.zeros(nq, dtype=torch.int32, device=dev) if counts else None)
    return np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32), (np.zeros(nq, np.int32) if counts else None)


class Bm25:
    """A resident lexical/bm25 MemoryIndex (vg_bm25): CSR postings, doc lengths and the doc -> id map.  The tokeniser, the
    string -> term id dictionary and the idf (math.Log) stay the host's; posting lists are in strictly ascending doc order
    (host arrays are checked).  Writes reach it through update(), which rewrites the image on the device; empty() makes
    an index that only updates fill, export() copies the image out."""

    def __init__(self, ctx: Context, term_off, post_doc, post_tf, doc_len, total_length: int, doc_count: int, doc_to_id=None):
        self._lib = ctx._lib
        self._ctx = ctx
        to, pto = _ptr(term_off, np.int64)
        self.n_terms = (to.numel() if _is_torch(to) else to.size) - 1
        dl, pdl = _ptr(doc_len, np.uint32)
        self.n_docs = dl.numel() if _is_torch(dl) else dl.size
        pd, ppd = _ptr(post_doc, np.uint32)
        pt, ppt = _ptr(post_tf, np.uint32)
        if (pd.numel() if _is_torch(pd) else pd.size) != (pt.numel() if _is_torch(pt) else pt.size):
            raise ValueError("Bm25: post_doc and post_tf hold one entry per posting each")
        di, pdi = _ptr(doc_to_id, np.uint32, self.n_docs) if doc_to_id is not None else (None, None)
        if self.n_terms < 0:
            raise ValueError("Bm25: term_off has n_terms + 1 entries")
        h = C.c_void_p()
        check(self._lib.vg_bm25_create(ctx._h, C.c_int64(self.n_docs), C.c_int64(self.n_terms), pto, ppd, ppt, pdl, C.c_int64(total_length),
                                       C.c_int64(doc_count), pdi, C.byref(h)))
        self._h = h
        self.mapped = doc_to_id is not None

    @classmethod
    def empty(cls, ctx: Context, with_doc_to_id: bool = False):
        """vg_bm25_create_empty: an index without docs or terms that update() fills; it answers nothing until then.
        with_doc_to_id: results are reported through the ids update() is given."""
        self = cls.__new__(cls)
        self._lib, self._ctx, self.n_terms, self.n_docs, self.mapped = ctx._lib, ctx, 0, 0, bool(with_doc_to_id)
        h = C.c_void_p()
        check(self._lib.vg_bm25_create_empty(ctx._h, C.c_int32(1 if with_doc_to_id else 0), C.byref(h)))
        self._h = h
        return self

    def update(self, del_docs, add_docs, add_len, add_off, add_terms, add_tf, n_docs: int, n_terms: int, total_length: int, doc_count: int,
               add_ids=None, stream=None):
        """vg_bm25_update: delete the docs del_docs, then add the docs add_docs (lengths add_len, reported under add_ids on an
        index with a doc_to_id map), doc i's postings being (add_terms[p], add_tf[p]) for p in add_off[i] : add_off[i + 1]
        (int64, one entry more than add_docs).  n_docs / n_terms: the index's sizes afterwards (they never shrink; term ids
        are stable, new terms are the ids behind the old ones); total_length / doc_count as in the constructor.  numpy or
        torch arrays, each on its own; None or an empty array for a side that is not wanted.  A failed call (VecgoHipError)
        leaves the index as it was."""
        def side(x, dtype):
            if x is None:
                return None, None, 0
            a, p = _ptr(x, dtype)
            n = a.numel() if _is_torch(a) else a.size
            return a, (p if n else None), n
        dd, pdd, n_del = side(del_docs, np.uint32)
        ad, pad, n_add = side(add_docs, np.uint32)
        al, pal, n_len = side(add_len, np.uint32)
        ai, pai, n_ids = side(add_ids, np.uint32)
        ao, pao, n_off = side(add_off, np.int64)
        at, pat, n_at = side(add_terms, np.uint32)
        af, paf, n_af = side(add_tf, np.uint32)
        if n_len != n_add or (n_add and n_off != n_add + 1) or n_at != n_af or (add_ids is not None and n_add and n_ids != n_add):
            raise ValueError("Bm25.update: add_len (and add_ids) hold one entry per added doc, add_off one more, add_terms and add_tf one per posting")
        if add_ids is not None and n_add == 0:
            pai = None
        check(self._lib.vg_bm25_update(self._h, pdd, C.c_int64(n_del), pad, pal, pai if add_ids is not None else None, C.c_int64(n_add),
                                       pao if n_add else None, pat, paf, C.c_int64(n_docs), C.c_int64(n_terms), C.c_int64(total_length),
                                       C.c_int64(doc_count), _stream_ptr(stream)))
        self.n_docs, self.n_terms = n_docs, n_terms

    def export(self, stream=None):
        """vg_bm25_export: the resident image as numpy arrays (term_off int64, post_doc, post_tf, doc_len, doc_to_id or None)"""
        st = self.stats()
        term_off = np.empty(st["terms"] + 1, np.int64)
        post_doc, post_tf = np.empty(st["postings"], np.uint32), np.empty(st["postings"], np.uint32)
        doc_len = np.empty(st["docs"], np.uint32)
        doc_to_id = np.empty(st["docs"], np.uint32) if self.mapped else None
        check(self._lib.vg_bm25_export(self._h, C.c_void_p(term_off.ctypes.data), C.c_void_p(post_doc.ctypes.data), C.c_void_p(post_tf.ctypes.data),
                                       C.c_void_p(doc_len.ctypes.data), C.c_void_p(doc_to_id.ctypes.data) if self.mapped else None,
                                       _stream_ptr(stream)))
        return term_off, post_doc, post_tf, doc_len, doc_to_id

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vg_bm25_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        """{docs, terms, postings, bytes} of the resident index (vg_bm25_stats)"""
        v = [C.c_int64(0) for _ in range(4)]
        check(self._lib.vg_bm25_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("docs", "terms", "postings", "bytes"), (x.value for x in v)))

    def replayed(self, stream=None) -> int:
        """vg_bm25_replayed: the queries since the index was made whose ties sent them through the reference's heap"""
        r = C.c_int64(0)
        check(self._lib.vg_bm25_replayed(self._h, C.byref(r), _stream_ptr(stream)))
        return r.value

    def search(self, q_term_off, q_terms, q_idf, k: int, out=None, stream=None):
        """MemoryIndex.Search for a batch (vg_bm25_search): query q's term ids q_terms[q_term_off[q] : q_term_off[q + 1]] with
        one float64 idf each (the caller's math.Log).  Returns (ids uint32 [nq, k] through doc_to_id, scores float32 [nq, k]
        best first, counts int32 [nq]); the tail is INVALID_ID / -inf.  numpy or torch, each on its own; out: the three
        arrays to fill.  k <= 16384, at most 64 terms per query."""
        qo, pqo = _ptr(q_term_off, np.int32)
        nq = (qo.numel() if _is_torch(qo) else qo.size) - 1
        if nq < 0:
            raise ValueError("Bm25.search: q_term_off has nq + 1 entries")
        qt, pqt = _ptr(q_terms, np.uint32)
        nt = qt.numel() if _is_torch(qt) else qt.size
        qi, pqi = _ptr_f64(q_idf, nt)
        ids, scores, counts = _result_buffers(out, nq, k, qo, self._ctx.device)
        i, pi = _ptr(ids, np.uint32, nq * k)
        s, ps = _ptr(scores, np.float32, nq * k)
        c, pc = _ptr(counts, np.int32, nq)
        if i is not ids or s is not scores or c is not counts:
            raise ValueError("Bm25.search: out must be contiguous arrays of uint32 / float32 / int32")
        check(self._lib.vg_bm25_search(self._h, pqo, pqt if nt else None, pqi if nt else None, C.c_int64(nq), C.c_int32(k), pi, ps, pc,
                                       _stream_ptr(stream)))
        return ids, scores, counts


def rrf_fuse(ctx: Context, a_ids, a_counts, b_ids, b_counts, k: int, rrf_k: int = 60, out=None, stream=None):
    """The Reciprocal Rank Fusion of Engine.HybridSearch (vg_rrf_fuse; engine.go:1560-1602) for a batch: a_ids / b_ids uint32
    [nq, stride] with a_counts / b_counts int32 [nq] entries each (None for a side: empty lists); rank r of A sets
    1 / float32(rrf_k + r + 1), every rank of B adds it.  Returns (ids [nq, k], scores [nq, k] best first, ties by ascending
    id, counts int32 [nq]).  At most 16384 entries per query in both lists together."""
    def side(ids, counts, what):
        if ids is None or counts is None:
            return None, None, None, None, 0, None
        if ids.ndim != 2:
            raise ValueError(f"rrf_fuse: {what} ids are [nq, stride]")
        i, pi = _ptr(ids, np.uint32)
        c, pc = _ptr(counts, np.int32, ids.shape[0])
        return i, pi, c, pc, int(ids.shape[1]), int(ids.shape[0])
    a, pa, ca, pca, sa, na = side(a_ids, a_counts, "a")
    b, pb, cb, pcb, sb, nb = side(b_ids, b_counts, "b")
    if na is None and nb is None:
        raise ValueError("rrf_fuse: both sides are None")
    nq = na if na is not None else nb
    if nb is not None and na is not None and na != nb:
        raise ValueError(f"rrf_fuse: a holds {na} queries, b {nb}")
    ids, scores, counts = _result_buffers(out, nq, k, a if a is not None else b, ctx.device)
    i, pi = _ptr(ids, np.uint32, nq * k)
    s, ps = _ptr(scores, np.float32, nq * k)
    c, pc = _ptr(counts, np.int32, nq)
    if i is not ids or s is not scores or c is not counts:
        raise ValueError("rrf_fuse: out must be contiguous arrays of uint32 / float32 / int32")
    check(ctx._lib.vg_rrf_fuse(ctx._h, C.c_int64(nq), pa, pca, C.c_int64(sa), pb, pcb, C.c_int64(sb), C.c_int32(rrf_k), C.c_int32(k), pi, ps, pc,
                               _stream_ptr(stream)))
    return ids, scores, counts


def hybrid_search(index: Index, bm: Bm25, queries, q_term_off, q_terms, q_idf, k: int, rrf_k: int = 60, stream=None):
    """Engine.HybridSearch for a batch over one resident segment (engine.go:1538-1602): the vector top-max(2k, 50) of
    index.search_flat and the BM25 top-max(2k, 50) of bm.search, fused by rrf_fuse, all on one stream; the two legs' lists
    never leave the device.  bm's doc_to_id maps docs to the index's row ids.  queries: float32 [nq, dim], numpy or torch.
    Returns (ids, scores, counts) as torch tensors on the device."""
    if torch is None:
        raise RuntimeError("hybrid_search keeps its intermediate lists in torch device tensors")
    dev = f"cuda:{index.ctx.device}"
    vk = max(2 * k, 50)
    nq = _rows(queries, index.dim)
    q = queries if _is_torch(queries) and queries.is_cuda else torch.as_tensor(np.ascontiguousarray(queries, np.float32)).to(dev)
    with torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else _null_ctx():
        v_ids = torch.empty((nq, vk), dtype=torch.int32, device=q.device)
        v_sc = torch.empty((nq, vk), dtype=torch.float32, device=q.device)
        index.search_flat(q, vk, out=(v_ids, v_sc), stream=stream)
        v_cnt = torch.full((nq,), vk, dtype=torch.int32, device=q.device)   # (search_flat pads with INVALID_ID, which the fusion skips)
        l_out = (torch.empty((nq, vk), dtype=torch.int32, device=q.device), torch.empty((nq, vk), dtype=torch.float32, device=q.device),
                 torch.zeros(nq, dtype=torch.int32, device=q.device))
        l_ids, _, l_cnt = bm.search(q_term_off, q_terms, q_idf, vk, out=l_out, stream=stream)
        out = (torch.empty((nq, k), dtype=torch.int32, device=q.device), torch.empty((nq, k), dtype=torch.float32, device=q.device),
               torch.zeros(nq, dtype=torch.int32, device=q.device))
        return rrf_fuse(index.ctx, v_ids, v_cnt, l_ids, l_cnt, k, rrf_k=rrf_k, out=out, stream=stream)


class _null_ctx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False
