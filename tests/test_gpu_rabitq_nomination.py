"""vg_index_enable_rabitq_nomination: vg_search_rabitq batches through the int8 matrix-core nomination (k_rabitq_nominate.hip).  The
GEMM multiplies the sign bits as +-1 int8 and gets every pair's Hamming distance exact; its epilogue lists the rows whose score may
be at or below the query's threshold (the sel-th best score of every 64th 64-row tile) behind a conservative screen; the verify
re-scores the listed rows with popcount and the reference's formula and proves the list complete; what it cannot prove goes to the
scan.  Results are the scan's and the oracle's, ids and score BITS.  Every case needs the new entry point.

The rule the cases restate (k_rabitq_nominate.hip's head): sampled rows = the rows of the 64-row tiles t with t % 64 == 0, for an
index of more than 64 tiles (else no sample: tau = +Inf, every row listed); tau = the nominate_sel_k(k)-th best sampled score (8 up
to k = 48, 16 up to 128, 32 up to 256); a query's list holds 4096 keys."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks

pytestmark = pytest.mark.gpu

SCOPE = "rabitq_nom_gemm"
CAP = 4096


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


@pytest.fixture
def nominate_always():
    """no crossover (the tests' segments are small), and the verify checks every listed Hamming distance against its popcount"""
    hooks.set_hook("VG_RABITQ_NOM_ALWAYS", 1)
    hooks.set_hook("VG_RABITQ_NOM_CHECK", 1)
    yield
    hooks.set_hook("VG_RABITQ_NOM_ALWAYS", 0)
    hooks.set_hook("VG_RABITQ_NOM_CHECK", 0)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def _same_nan(a, b):
    return np.array_equal(a[0], b[0]) and bool(np.all((bits(a[1]) == bits(b[1])) | (np.isnan(a[1]) & np.isnan(b[1]))))


def _launches(ctx, search):
    """search()'s result and how often the nomination GEMM ran in it"""
    ctx.profile_enable(True)
    try:
        ctx.profile_read(SCOPE)
        r = search()
        return r, ctx.profile_read(SCOPE)[0]
    finally:
        ctx.profile_enable(False)


def _index(vg, ctx, codes, dim):
    idx = vg.Index(ctx, codes.shape[0], dim)
    idx.set_rabitq_codes(codes)
    return idx


def _oracle_equal(codes, dim, q, k, got, which):
    for i in which:
        eid, esc = o.flat_search_rabitq(codes, dim, q[i], k)
        assert np.array_equal(got[0][i, :eid.size], eid), i
        assert np.array_equal(bits(got[1][i, :eid.size]), bits(esc)), i


def sel_k(k):
    return 8 if k <= 48 else 16 if k <= 128 else 32


def distances(codes, dim, q):
    """[nq, n] RaBitQ distances, float32 in the reference's operation order (rabitq.go:170-175), from the codes and the queries'
    own codes; tied to the oracle's rabitq_distance on a few pairs"""
    nb = (dim + 63) // 64 * 8
    qc = o.rabitq_encode_batch(q, dim)
    words, qwords = np.ascontiguousarray(codes[:, :nb]).view(np.uint64), np.ascontiguousarray(qc[:, :nb]).view(np.uint64)
    yn, qn = np.ascontiguousarray(codes[:, nb:]).view(np.float32)[:, 0], np.ascontiguousarray(qc[:, nb:]).view(np.float32)[:, 0]
    out = np.empty((len(q), len(codes)), np.float32)
    with np.errstate(all="ignore"):
        for i in range(len(q)):
            h = np.bitwise_count(words ^ qwords[i]).sum(1).astype(np.float32)
            t1 = (qn[i] - yn).astype(np.float32)
            t2 = (np.float32(4.0) * qn[i]).astype(np.float32) * yn
            t2 = (t2 / np.float32(dim)).astype(np.float32) * h
            out[i] = (t1 * t1).astype(np.float32) + t2.astype(np.float32)
    rng = np.random.default_rng(1)
    for i, r in zip(rng.integers(0, len(q), 12), rng.integers(0, len(codes), 12)):
        assert bits(out[i, r]) == bits(o.rabitq_distance(q[i], codes[r])), (i, r)
    return out


def rows_at_or_below_threshold(codes, dim, q, k):
    """per query: how many rows score at or below the threshold the rule above sets (the list the GEMM has to produce, before the
    screen's few false passes)"""
    d = distances(codes, dim, q)
    n = len(codes)
    sample = np.flatnonzero((np.arange(n) // 64) % 64 == 0)
    tau = np.sort(d[:, sample], axis=1)[:, sel_k(k) - 1]
    return (d <= tau[:, None]).sum(1)


def corpus(kind, n, dim, nq, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        x = rng.standard_normal((n, dim)).astype(np.float32)
        q = rng.standard_normal((nq, dim)).astype(np.float32)
    else:
        cent = rng.standard_normal((30, dim)).astype(np.float32) * 2
        x = (cent[rng.integers(0, 30, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.5).astype(np.float32)
        q = (cent[rng.integers(0, 30, nq)] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.5).astype(np.float32)
    return x, q


def planted(kind, n, dim, nq, seed):
    """codes with ten identical rows, an all-ones and an all-zero code, the last row equal to an early one; queries equal to rows"""
    x, q = corpus(kind, n, dim, nq, seed)
    nb = (dim + 63) // 64 * 8
    x[n - 1] = x[7]
    q[1], q[2], q[3] = x[100], x[n - 1], x[200]
    codes = o.rabitq_encode_batch(x, dim)
    codes[100:110] = codes[100]
    codes[200, :nb], codes[201, :nb] = 0xFF, 0x00
    return codes, q


SHAPES = [(20000, 768, 300, 10),    # six K steps, two query tiles, the last row tile partial
          (9000, 128, 300, 10),     # one K step
          (4097, 64, 130, 10),      # half a K step of real bits; the first size with a sample
          (5000, 100, 200, 100),    # dim % 64 != 0: pad bits
          (12000, 128, 257, 256),   # k at the limit; a query tile holding one query
          (30000, 256, 200, 100),
          (70000, 64, 300, 10),     # more tiles than workgroups
          (300, 16, 129, 5)]        # no sample: everything listed


@pytest.mark.parametrize("kind", ["normal", "clustered"])
@pytest.mark.parametrize("n,dim,nq,k", SHAPES)
def test_parity_with_scan_and_oracle(vg, ctx, nominate_always, n, dim, nq, k, kind):
    codes, q = planted(kind, n, dim, nq, n + dim)
    idx = _index(vg, ctx, codes, dim)
    plain = idx.search_rabitq(q, k)
    idx.enable_rabitq_nomination(True)
    got, launches = _launches(ctx, lambda: idx.search_rabitq(q, k))
    assert launches >= 1, "the batch kept the scan"
    assert _same(plain, got)
    _oracle_equal(codes, dim, q, k, got, range(nq) if n * nq <= 4000000 else list(range(8)) + list(range(8, nq, 7)))
    on, held, rescanned, mismatched = idx.rabitq_nomination_info()
    assert (on, held) == (1, 0)
    assert mismatched == 0
    if n > CAP:     # the shape without a sample lists everything: no precondition, nothing to count
        below = rows_at_or_below_threshold(codes, dim, q, k)
        print(f"n={n} dim={dim} nq={nq} k={k} {kind}: rows at or below tau {below.min()} .. {below.max()}, rescanned {rescanned}")
        assert below.max() <= (CAP if k == 256 else CAP // 2) and below.min() >= k      # the inputs: every list fits and proves
        assert rescanned == 0


def test_every_slot_and_bit_decides(vg, ctx, nominate_always):
    """dim 256 (two K steps), codes written as bytes, equal norms.  Query j has its own random bits; a target row with exactly
    those bits sits at a row slot of its own in one 256-row tile, a decoy with bit j flipped at another slot of another tile: every
    one of the 256 query slots, 256 row slots and 256 bit positions decides one (target, decoy) pair.  k = 2: the oracle's."""
    rng = np.random.default_rng(8)
    n, dim, nq, nb = 256 * 33, 256, 256, 32
    norm = np.frombuffer(np.float32(16.0).tobytes(), np.uint8)          # |+-1 vector of 256| = 16
    codes = np.empty((n, nb + 4), np.uint8)
    codes[:, :nb] = rng.integers(0, 256, (n, nb))
    codes[:, nb:] = norm
    qbits = rng.integers(0, 2, (nq, dim)).astype(np.uint8)
    q = (qbits.astype(np.float32) * 2 - 1).astype(np.float32)           # Encode: v >= 0 sets the bit
    target, decoy = np.empty(nq, np.int64), np.empty(nq, np.int64)
    for j in range(nq):
        target[j] = 256 * (1 + j % 16) + (j + 37) % 256
        decoy[j] = 256 * (17 + j % 16) + (5 * j + 11) % 256
        b = np.packbits(qbits[j], bitorder="little")
        codes[target[j], :nb] = b
        flipped = qbits[j].copy()
        flipped[j] ^= 1
        codes[decoy[j], :nb] = np.packbits(flipped, bitorder="little")
    assert len(set(target)) == nq and len(set(decoy)) == nq and len(set(target % 256)) == 256 and len(set(decoy % 256)) == 256
    assert np.array_equal(o.rabitq_encode_batch(q, dim)[:, :nb], codes[target, :nb])
    idx = _index(vg, ctx, codes, dim)
    plain = idx.search_rabitq(q, 2)
    idx.enable_rabitq_nomination(True)
    got, launches = _launches(ctx, lambda: idx.search_rabitq(q, 2))
    assert launches >= 1 and _same(plain, got)
    assert np.array_equal(got[0][:, 0], target.astype(np.uint32)) and np.array_equal(got[0][:, 1], decoy.astype(np.uint32))
    assert np.array_equal(got[1], np.tile(np.float32([0.0, 4.0]), (nq, 1)))     # h = 0 and h = 1: 4 * 16 * 16 / 256
    _oracle_equal(codes, dim, q, 2, got, range(nq))
    on, held, rescanned, mismatched = idx.rabitq_nomination_info()
    assert mismatched == 0 and rescanned == 0


def test_overflow_falls_back_to_the_scan(vg, ctx, nominate_always):
    """6000 identical codes: every row ties at the threshold, every list overflows, every query is answered by the scan"""
    rng = np.random.default_rng(3)
    n, dim, nq, k = 6000, 64, 130, 10
    codes = np.tile(o.rabitq_encode_batch(rng.standard_normal((1, dim)).astype(np.float32), dim), (n, 1))
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = _index(vg, ctx, codes, dim)
    plain = idx.search_rabitq(q, k)
    idx.enable_rabitq_nomination(True)
    got, launches = _launches(ctx, lambda: idx.search_rabitq(q, k))
    assert launches >= 1 and _same(plain, got)
    assert np.array_equal(got[0], np.tile(np.arange(k, dtype=np.uint32), (nq, 1)))      # ties in id order
    assert idx.rabitq_nomination_info()[2:] == (nq, 0)
    _oracle_equal(codes, dim, q, k, got, (0, nq - 1))


def test_non_finite_values(vg, ctx, nominate_always):
    """a NaN norm, an Inf norm, a query holding an Inf: on = off, bit for bit.  A NEGATIVE stored norm: the index keeps the scan"""
    rng = np.random.default_rng(11)
    n, dim, nq, k, nb = 5000, 64, 130, 10, 8
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = (x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, dim)).astype(np.float32)).astype(np.float32)
    base = o.rabitq_encode_batch(x, dim)
    for what in ("inf_query", "nan_norm", "inf_norm", "negative_norm"):
        codes, qq = base.copy(), q.copy()
        if what == "inf_query":
            qq[5, 3] = np.inf
        elif what == "nan_norm":
            codes[70, nb:] = np.frombuffer(np.float32(np.nan).tobytes(), np.uint8)
            qq[5, 3] = np.inf
        elif what == "inf_norm":
            codes[4000, nb:] = np.frombuffer(np.float32(np.inf).tobytes(), np.uint8)
        else:
            codes[33, nb:] = np.frombuffer(np.float32(-1.5).tobytes(), np.uint8)
        idx = _index(vg, ctx, codes, dim)
        plain = idx.search_rabitq(qq, k)
        idx.enable_rabitq_nomination(True)
        got, launches = _launches(ctx, lambda: idx.search_rabitq(qq, k))
        assert _same_nan(plain, got), what
        assert idx.rabitq_nomination_info()[3] == 0
        if what == "negative_norm":
            assert launches == 0 and idx.rabitq_nomination_info()[:3] == (1, 0, 0)
        else:
            assert launches >= 1, what
        if what == "inf_query":
            assert 1 <= idx.rabitq_nomination_info()[2] <= 1 + nq // 20      # the Inf query fails its proof; hardly any other
            _oracle_equal(codes, dim, qq, k, got, (0, 5, nq - 1))


def test_life_cycle_and_batches_the_mode_does_not_take(vg, ctx):
    rng = np.random.default_rng(5)
    n, dim, nq, k = 9000, 128, 200, 10
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    codes = o.rabitq_encode_batch(x, dim)
    idx = _index(vg, ctx, codes, dim)
    assert idx.rabitq_nomination_info() == (0, 0, 0, 0)
    plain = [idx.search_rabitq(q[:128], k), idx.search_rabitq(q, 257), idx.search_rabitq(q, k), idx.search_rabitq(q[:1], k)]
    idx.enable_rabitq_nomination(True)
    assert idx.rabitq_nomination_info() == (1, 0, 0, 0)
    # without the hook 200 x 9000 pairs lie below the crossover
    got, launches = _launches(ctx, lambda: idx.search_rabitq(q, k))
    assert launches == 0 and _same(plain[2], got)
    hooks.set_hook("VG_RABITQ_NOM_ALWAYS", 1)
    try:
        got, launches = _launches(ctx, lambda: [idx.search_rabitq(q[:128], k), idx.search_rabitq(q, 257), None, idx.search_rabitq(q[:1], k)])
        assert launches == 0 and all(_same(a, b) for a, b in zip(plain, got) if b is not None)
        got, launches = _launches(ctx, lambda: idx.search_rabitq(q, k))
        assert launches >= 1 and _same(plain[2], got)
        # identical codes: every query is rescanned; enabling again zeroes the count
        same = np.tile(codes[:1], (6000, 1))
        sidx = _index(vg, ctx, same, dim)
        sidx.enable_rabitq_nomination(True)
        sidx.search_rabitq(q, k)
        assert sidx.rabitq_nomination_info() == (1, 0, nq, 0)
        sidx.enable_rabitq_nomination(True)
        assert sidx.rabitq_nomination_info() == (1, 0, 0, 0)
        sidx.enable_rabitq_nomination(False)
        assert sidx.rabitq_nomination_info() == (0, 0, 0, 0)
        assert _launches(ctx, lambda: sidx.search_rabitq(q, k))[1] == 0
        # new codes drop the mode
        idx.set_rabitq_codes(o.rabitq_encode_batch(rng.standard_normal((n, dim)).astype(np.float32), dim))
        assert idx.rabitq_nomination_info() == (0, 0, 0, 0)
        assert _launches(ctx, lambda: idx.search_rabitq(q, k))[1] == 0
    finally:
        hooks.set_hook("VG_RABITQ_NOM_ALWAYS", 0)
    # refusals: no codes (VG_ERR_NOT_READY)
    with pytest.raises(vg.VecgoHipError) as e:
        vg.Index(ctx, 10, dim).enable_rabitq_nomination(True)
    assert e.value.status == -9 and "no RaBitQ codes" in e.value.message


def test_reorder_leaves_the_mode_correct(vg, ctx, nominate_always):
    """vg_vamana_reorder_bfs permutes the codes, tiles and norms; the mode holds nothing per row and stays on and right"""
    rng = np.random.default_rng(21)
    n, dim, r, nq, k = 6000, 128, 24, 160, 10
    x = rng.standard_normal((n, dim)).astype(np.float32) * (1.0 + rng.random((n, 1)).astype(np.float32))
    q = (x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, dim)).astype(np.float32)).astype(np.float32)
    codes = o.rabitq_encode_batch(x, dim)
    g = rng.integers(0, n, (n, r)).astype(np.uint32)
    g[rng.random((n, r)) < 0.3] = 0xFFFFFFFF
    idx = _index(vg, ctx, codes, dim)
    idx.set_vectors(x)
    idx.enable_rabitq_nomination(True)
    idx.set_vamana_graph(g, n // 3)
    perm, inv = idx.reorder_vamana_bfs()
    assert idx.rabitq_nomination_info()[0] == 1 and not np.array_equal(perm, np.arange(n))
    got, launches = _launches(ctx, lambda: idx.search_rabitq(q, k))
    assert launches >= 1 and idx.rabitq_nomination_info()[3] == 0
    assert _same(_index(vg, ctx, codes[perm], dim).search_rabitq(q, k), got)


def test_device_queries_at_an_odd_offset_on_a_callers_stream(vg, ctx, nominate_always):
    torch = pytest.importorskip("torch")
    n, dim, nq, k = 9000, 128, 300, 10
    codes, q = planted("normal", n, dim, nq, n + dim)
    idx = _index(vg, ctx, codes, dim)
    plain = idx.search_rabitq(q, k)
    idx.enable_rabitq_nomination(True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        buf = torch.zeros(nq * dim + 3, dtype=torch.float32, device="cuda")
        dq = buf[3:].view(nq, dim)                       # 12 bytes past a 16-byte boundary
        dq.copy_(torch.from_numpy(q))
        oi = torch.empty(nq * k + 1, dtype=torch.int32, device="cuda")[1:].view(nq, k)
        osc = torch.empty(nq * k + 1, dtype=torch.float32, device="cuda")[1:].view(nq, k)
        _, launches = _launches(ctx, lambda: idx.search_rabitq(dq, k, out=(oi, osc), stream=s))
    s.synchronize()
    assert launches >= 1
    assert np.array_equal(oi.cpu().numpy().view(np.uint32), plain[0]) and np.array_equal(bits(osc.cpu().numpy()), bits(plain[1]))
    assert idx.rabitq_nomination_info()[2:] == (0, 0)
