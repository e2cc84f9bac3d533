"""Inputs that put the seams of build_link_kernel (k_hnsw_build.hip) under the data: back-link chains of hundreds of
records on one row, records that must change the row at lane 0 and lane 63 of a later chunk, whole chunks of far records,
rows whose members tie (the replayed heap, the `stable` shortcut), ties under Dot and Cosine, and ef_construction at its
limits.

Plain builders with seeded, frozen arrays: tests/test_hnsw_build_seams_cpu.py proves against the oracle's event log
(oracle.hnsw_build(..., events=True)) that every case reaches what it is named for; tests/test_gpu_hnsw_build_seams.py
compares the library's graph with the oracle's on them.

A hub: row 0 is nearer to every other row than they are to each other, so every node of a batch links back to row 0 and
row 0's chain in a batch is the batch itself — chain position = position in the batch.  growth_div = 1 makes the batches
1, 2, 4, ... up to max_batch, so the batch that starts at row `done` is known in advance (batches())."""
import collections
import functools

import numpy as np

from oracle import oracle as o

Case = collections.namedtuple("Case", "name base dim m ef metric max_batch growth_div")


def batches(n, max_batch, growth_div):
    """(first row, size) of every batch of the one-call schedule: clamp(done / growth_div, 1, max_batch) from done = 1"""
    out, done = [], 1
    while done < n:
        b = min(max(done // growth_div, 1), max_batch, n - done)
        out.append((done, b))
        done += b
    return out


def _directions(rng, n, dim):
    u = rng.standard_normal((n, dim))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _hub_rows(seed, n, dim, early=512, planted=(), late=(1.15, 1.3), mirror=(), members=0, pairs=()):
    """float64 rows: row 0 zero; rows < early on a shell of radius 1.0..1.3, later rows at `late` — farther than every member
    row 0 keeps from the early ones, so a later record is one the link kernel may skip; planted {row: radius} puts a nearer row
    where a record has to change row 0; mirror {row: rank} makes the row the negative of the early row with that rank by
    radius: exactly as far from row 0.
    members, pairs: rows 1..members have the radii 0.6..1.1 in ascending order and every other row is at 1.2..1.3, so they are
    row 0's list once they are in; for every rank in pairs the member of rank + 1 is the negative of the member of that rank:
    equally far from row 0 in bits (the same squares in the same order)."""
    rng = np.random.default_rng(seed)
    u = _directions(rng, n, dim)
    r = np.where(np.arange(n) < early, rng.uniform(1.0, 1.3, n), rng.uniform(late[0], late[1], n))
    if members:
        r = rng.uniform(1.2, 1.3, n)
        r[1:1 + members] = np.linspace(0.6, 1.1, members)
    for row, radius in dict(planted).items():
        r[row] = radius
    x = u * r[:, None]
    for rank in pairs:
        x[2 + rank] = -x[1 + rank]
    by_radius = 1 + np.argsort(r[1:early], kind="stable")
    for row, rank in dict(mirror).items():
        x[row] = -x[by_radius[rank]]
    x[0] = 0.0
    return x


def _frozen(x):
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


# work records of the batch that starts at row 512 (max_batch 300: rows 512..811), by chain position on row 0: lane 0 and
# lane 63 of chunks 1 and 2.  Chunk 3 (192..255) is far records only and chunk 4 (256..299) is ragged.
HUB_WORK = {512 + 64: 0.9, 512 + 127: 0.8, 512 + 128: 0.7, 512 + 191: 0.6}
# hub-ties: nearer rows late in the run, each one changes the tied row and resets `stable`
TIES_WORK = {512 + 100: 0.5, 812 + 70: 0.45, 1112 + 5: 0.4}


def _dot_hub(seed, n, dim, planted):
    """A hub under Dot with negative distances: the shell rows get one more coordinate w = sqrt(4 - r^2) (all norms 2) and
    row 0 is 8 on that axis, so d(row 0, i) = -8 w_i orders the rows as their radius does and is below every d(i, j) >= -4."""
    x = _hub_rows(seed, n, dim - 1, planted=planted)
    w = np.sqrt(4.0 - (x * x).sum(1))
    y = np.concatenate([x, w[:, None]], 1)
    y[0] = 0.0
    y[0, -1] = 8.0
    return y


def _cosine_hub(seed, n, dim, planted, members, pairs):
    """Unit rows: row 0 is the last axis, row i = (sin(a_i) u_i, cos(a_i)); rows 1..members at a_i = 20..27 degrees in
    ascending order, every other row at 28..35, planted {row: degrees} nearer.  For every rank in pairs the member of rank + 1
    is (-sin(a) u, cos(a)) of the member (sin(a) u, cos(a)) of that rank: equally far from row 0 in bits."""
    rng = np.random.default_rng(seed)
    u = _directions(rng, n, dim - 1)
    a = rng.uniform(28.0, 35.0, n)
    a[1:1 + members] = np.linspace(20.0, 27.0, members)
    for row, deg in planted.items():
        a[row] = deg
    a = np.deg2rad(a)
    y = np.concatenate([u * np.sin(a)[:, None], np.cos(a)[:, None]], 1).astype(np.float32)
    for rank in pairs:
        y[2 + rank, :-1] = -y[1 + rank, :-1]
        y[2 + rank, -1] = y[1 + rank, -1]
    y[0] = 0.0
    y[0, -1] = 1.0
    return y


def _cube(seed, n, dim=12):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2, (n, dim)) * 2.0 - 1.0
    x[0] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def cases():
    L2, COS, DOT = o.METRIC_L2, o.METRIC_COSINE, o.METRIC_DOT
    out = []

    def add(name, base, m, ef, metric=L2, max_batch=300, growth_div=1):
        base = _frozen(base)
        out.append(Case(name, base, base.shape[1], m, ef, metric, max_batch, growth_div))

    # chains of 256 and 300 on row 0 with work at chain positions 64, 127, 128, 191, a far chunk, a ragged far tail
    # ... and in the next batch (rows 812..1111) a record exactly as far as row 0's last member: after the four planted rows
    # the row is they and its 2M - 4 nearest early rows
    add("hub-m8", _hub_rows(1, 1400, 32, planted=HUB_WORK, mirror={812 + 130: 16 - 4 - 1}), 8, 64)
    add("hub-m32", _hub_rows(2, 1400, 64, planted=HUB_WORK, mirror={812 + 130: 64 - 4 - 1}), 32, 100)   # degree 64
    # a full row of tied members that far records leave as it is (`stable`), changed three times on the way
    # (the reference's heap hands a tied pair back in the order it got it at some ranks and swapped at others — swapped
    # among the four nearest — so where the pairs stand decides whether the row settles.  At degree 64 these fifteen pairs
    # settle until the second planted row has moved them two ranks down; from there every far record changes the row)
    add("hub-ties-m8", _hub_rows(3, 1400, 32, planted=TIES_WORK, members=16, pairs=(6, 8, 10, 12, 14)), 8, 64)
    add("hub-ties-m32", _hub_rows(4, 1400, 64, planted=TIES_WORK, members=64,
                                  pairs=tuple(range(20, 30, 2)) + tuple(range(36, 46, 2)) + tuple(range(52, 62, 2))), 32, 100)
    # one tied pair, row 0's two nearest members: every far record swaps the two, so the row never settles, and the build
    # ends on an odd number of swaps — a kernel that skipped those records would leave the pair the other way round
    add("swap-m8", _hub_rows(15, 700, 32, members=16, pairs=(0,)), 8, 64)
    add("swap-m32", _hub_rows(16, 701, 64, members=64, pairs=(0,)), 32, 100)
    # negative distances; ties under Cosine
    add("hub-dot", _dot_hub(5, 1400, 64, HUB_WORK), 8, 64, DOT)
    add("hub-cosine", _cosine_hub(16, 1400, 64, {**{r: 15.0 - i for i, r in enumerate(HUB_WORK)}, 812 + 70: 10.0}, 16,
                                  (6, 8, 10, 12, 14)), 8, 64, COS)
    # every distance ties: the replayed heap at degree 32 and 64, on upper levels, under Dot
    cube = _cube(7, 2000)
    add("cube-m16", cube, 16, 64, max_batch=400)
    add("cube-m32", cube, 32, 100, max_batch=400)
    add("cube-dot", cube, 16, 64, DOT, max_batch=400)
    # chain lengths 63 / 64 / 65 / 128 / 129 / 257: the batch sizes of the schedule and its last batch
    # (the batches grow 1, 2, 4, ... to max_batch; one batch of max_batch rows ends the build)
    for size in (63, 65, 129, 257):
        n = next(t0 + b for t0, b in batches(4 * size, size, 1) if b == size)
        add(f"len-{size}", _hub_rows(8 + size, n, 64, early=64), 8, 64, max_batch=size)
    # ef_construction at its limits: ef < M takes selectNeighborsSimple for every own row (rows stay appended, then fill in
    # the middle of a chain); M, M + 1 and 2M, 2M + 1 are the seams of the upper levels and of layer 0; 1024 = kBuildMaxEf
    ef_rows = _hub_rows(12, 900, 32, early=256)
    for ef in (1, 7, 8, 9, 16, 17, 1024):
        add(f"ef-{ef}", ef_rows, 8, ef)
    add("ef-1024-n1400", _hub_rows(13, 1400, 32), 8, 1024)
    # >= 1000 records on row 0 in one batch (rows 1024..2047): the rank sort's strides, the debug run's timed branch
    add("chain-1000", _hub_rows(14, 2100, 32, early=1024), 8, 64, max_batch=1200)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def oracle_build(name):
    """(l0, upper, entry_point, links, own) of the case, computed once"""
    c = case(name)
    return o.hnsw_build(c.base, c.dim, m=c.m, ef=c.ef, metric=c.metric, max_batch=c.max_batch, growth_div=c.growth_div,
                        events=True)


def chains(links):
    """{(batch, level, node): the row's events of that batch, in application order}"""
    order = np.lexsort((links["pos"], links["node"], links["level"], links["batch"]))
    s = links[order]
    key = np.stack([s["batch"], s["level"], s["node"].astype(np.int64)], 1)
    cut = np.nonzero((key[1:] != key[:-1]).any(1))[0] + 1
    return {tuple(int(v) for v in key[a]): s[a:b] for a, b in zip(np.r_[0, cut], np.r_[cut, len(s)])}
