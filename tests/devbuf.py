"""Device buffers the way a serving process hands them to the library (tests/test_gpu_device_buffers.py): views that sit at an
odd offset inside a larger allocation, and inputs whose producer is still running on the caller's stream."""
import numpy as np
import torch

_TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32,
             np.dtype(np.uint32): torch.int32}   # torch has no uint32: the same bits as int32


def _as_torch_host(array):
    a = np.ascontiguousarray(array)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype not in _TORCH_OF:
        raise TypeError(f"no device twin for dtype {a.dtype}")
    return torch.from_numpy(a)


def skew_bytes_of(array) -> int:
    """The smallest offset that keeps a buffer element-aligned and breaks its 16-byte alignment: one element."""
    return np.asarray(array).dtype.itemsize


def whole(array):
    """`array` as a whole device tensor: the allocator's alignment (at least 256 bytes)."""
    t = _as_torch_host(array).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def offset_like(array, skew_bytes):
    """A contiguous device view holding `array`, `skew_bytes` past the start of a flat allocation that is that much longer:
    element-aligned, not 16-byte aligned (byte buffers: not even 8-byte aligned).  vecgo_amd.api._ptr passes a contiguous
    view through unchanged, so the library sees exactly this address."""
    h = _as_torch_host(array)
    item = h.element_size()
    assert skew_bytes % item == 0 and 0 < skew_bytes < 16, (skew_bytes, item)
    skew = skew_bytes // item
    flat = torch.empty(h.numel() + skew, dtype=h.dtype, device="cuda")
    view = flat[skew:skew + h.numel()].view(h.shape)
    view.copy_(h)
    assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + skew_bytes
    assert view.data_ptr() % item == 0 and view.data_ptr() % 16 != 0, hex(view.data_ptr())
    if item == 1:
        assert view.data_ptr() % 8 != 0, hex(view.data_ptr())
    return view


def to_host(t):
    """numpy copy of a device tensor or a numpy array (waits for the stream work in front of the copy)"""
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def raw(x):
    """the bytes of a result, for bit-for-bit comparison whatever the dtype (uint32 ids travel as int32 in torch)"""
    return np.ascontiguousarray(to_host(x)).reshape(-1).view(np.uint8)


def poison_(t, value=None):
    """Overwrite a tensor in place on the current stream: NaN for floats, 0xFF bytes otherwise (or `value`)."""
    if value is not None:
        t.fill_(value)
    elif t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(0xFF)
    else:
        t.fill_(-1)
    return t


# The delay: a chain of dependent fp32 matrix products on the caller's stream.  Measured on an MI355X with events around
# the chain, after a warm-up chain on the same stream: DELAY_DIM = 4096, DELAY_MATMULS = 32 takes 29.1 ms (29.08 .. 29.32
# over ten runs; 24 products: 21.9 ms, too close to the floor).  The target is 20 .. 60 ms: an order of magnitude above an
# entry point's host-side enqueue, short enough for some ninety cases.
DELAY_DIM = 4096
DELAY_MATMULS = 32
_delay_state = {}


def _delay_buffers():
    if not _delay_state:
        w = torch.full((DELAY_DIM, DELAY_DIM), 1.0 / DELAY_DIM, dtype=torch.float32, device="cuda")  # keeps magnitudes
        _delay_state["w"] = w
        _delay_state["x"] = [torch.ones((DELAY_DIM, DELAY_DIM), dtype=torch.float32, device="cuda") for _ in range(2)]
    return _delay_state["w"], _delay_state["x"]


def enqueue_delay(stream, matmuls=None):
    """DELAY_MATMULS dependent products on `stream` (no allocation once the buffers exist)"""
    w, x = _delay_buffers()
    with torch.cuda.stream(stream):
        for i in range(DELAY_MATMULS if matmuls is None else matmuls):
            torch.mm(x[i & 1], w, out=x[(i + 1) & 1])


def time_delay(stream):
    """milliseconds the chain takes on `stream`, by events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    enqueue_delay(stream)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def late_inputs(stream, tensors, real_values, poisons=None):
    """Everything on `stream`: poison each tensor (NaN for floats, 0xFF for bytes; poisons[i] overrides), run the delay, then
    copy the real values in from the staging tensors (device to device) and record an event.  Until that event completes the
    tensors hold poison: a consumer is right only if it is ordered behind the copies on this stream.  Returns the event."""
    assert len(tensors) == len(real_values)
    with torch.cuda.stream(stream):
        for i, t in enumerate(tensors):
            poison_(t, None if poisons is None else poisons[i])
        enqueue_delay(stream)
        for t, r in zip(tensors, real_values):
            t.copy_(r, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev
