"""Finish of a GroupTable straight into shuffle partitions.

_C.groupby_compact_partition(tkeys, tabs, flags, nparts) is compared, on the
same table, with the order it replaces: _C.groupby_compact, the sentinel
row appended, then _C.hash_partition with seed 0.  Counts are equal; per
partition the keys are equal after sorting and the value columns are equal
bit for bit in that order (values are copied, never recomputed); and every
key sits in the partition hashing.hash_columns gives on the host.  Then
GroupTable.finish_partitioned through an overflow, and bs.Reduce end to
end with the switch on and off, against torch on the CPU.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NPARTS = [1, 2, 3, 8, 64, 1000]

# name -> (capacity, keys, rows, sentinel-key rows)
SHAPES = {
    "cap1024": (1024, 300, 2000, 0),
    "cap65536": (65536, 20000, 60000, 0),
    "one_key": (1024, 1, 1, 0),
    "empty": (1024, 0, 0, 0),
    "sentinel": (1024, 300, 2000, 5),
}
# name -> [(dtype, aggregation)]
VALUES = {
    "i64sum": [(torch.int64, "sum")],
    "i32min_f64max": [(torch.int32, "min"), (torch.float64, "max")],
    "f32sum_i64sum": [(torch.float32, "sum"), (torch.int64, "sum")],
}


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


def _column(dtype, n, g):
    if dtype.is_floating_point:
        return (torch.randn(n, generator=g, dtype=torch.float64) * 1e3).to(
            dtype)
    return torch.randint(-1000, 1000, (n,), generator=g, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _table(shape, values):
    """(tkeys, tabs, flags) of one filled table, built once and only read
    afterwards."""
    from bigslice_amd import kernels as k
    cap, nkeys, rows, nsent = SHAPES[shape]
    spec = VALUES[values]
    g = torch.Generator().manual_seed(cap + nkeys)
    tkeys = torch.full((cap + 1,), k.GB_SENTINEL, dtype=torch.int64,
                       device=DEV)
    codes = [k._AGG_CODES[a] for _, a in spec]
    tabs = [k._C.agg_identity(torch.empty(0, dtype=dt, device=DEV), c,
                              cap + 1) for (dt, _), c in zip(spec, codes)]
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    if rows:
        pool = torch.randint(-(1 << 62), 1 << 62, (nkeys,), generator=g)
        keys = pool[torch.randint(0, nkeys, (rows,), generator=g)]
        keys[:nkeys] = pool  # every key at least once
        keys[rows - nsent:] = k.GB_SENTINEL
        vals = [_column(dt, rows, g).to(DEV) for dt, _ in spec]
        k._C.groupby_insert(keys.to(DEV), vals, codes, tkeys, tabs, flags,
                            k.MAX_PROBES)
    assert flags.tolist() == [int(nsent > 0), 0]
    return tkeys, tabs, flags


def _bits(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _old_order(k, tkeys, tabs, flags, nparts):
    """(counts, columns in partition order) by compaction, then
    hash_partition."""
    cap = tkeys.shape[0] - 1
    cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
    outs = k._C.groupby_compact(tkeys, tabs, cursor)
    n = int(cursor.item())
    cols = [o[:n] for o in outs]
    if int(flags[0].item()):
        cols = [torch.cat([c, t[cap:cap + 1]])
                for c, t in zip(cols, [tkeys] + list(tabs))]
    if cols[0].shape[0] == 0:
        return [0] * nparts, cols
    cols, counts = k._C.hash_partition(
        [c.contiguous() for c in cols], [cols[0].contiguous()], nparts, 0)
    return counts.tolist(), cols


def _by_partition(cols, counts):
    """Per partition the columns on the CPU, rows ordered by key."""
    out, off = [], 0
    for c in counts:
        part = [col[off:off + c].cpu() for col in cols]
        o = torch.argsort(part[0])
        out.append([p[o] for p in part])
        off += c
    return out


def _check(k, shape, values, nparts):
    from bigslice_amd import hashing
    tkeys, tabs, flags = _table(shape, values)
    cap = tkeys.shape[0] - 1
    before = [t.clone() for t in [tkeys] + list(tabs)]
    outs, host = k._C.groupby_compact_partition(tkeys, tabs, flags, nparts)
    assert not host.is_cuda and host.dtype == torch.int64
    *counts, sentinel_seen, overflow = host.tolist()
    assert len(counts) == nparts and overflow == 0
    assert sentinel_seen == int(SHAPES[shape][3] > 0)
    want_counts, want_cols = _old_order(k, tkeys, tabs, flags, nparts)
    assert counts == want_counts
    assert sum(counts) == SHAPES[shape][1] + sentinel_seen
    assert all(o.shape[0] == cap + 1 for o in outs)
    got = _by_partition(outs, counts)
    want = _by_partition(want_cols, want_counts)
    for pi, (gp, wp) in enumerate(zip(got, want)):
        assert torch.equal(gp[0], wp[0])
        for gc, wc in zip(gp[1:], wp[1:]):
            assert gc.dtype == wc.dtype
            assert torch.equal(_bits(gc), _bits(wc))
        if gp[0].numel():
            h = hashing.hash_columns([gp[0]], 0).to(torch.int64)
            assert bool((((h & 0xFFFFFFFF) % nparts) == pi).all())
    # the table is only read
    for b, t in zip(before, [tkeys] + list(tabs)):
        assert torch.equal(_bits(b), _bits(t))


@pytest.mark.parametrize("nparts", NPARTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_int64_sum(kernels, shape, nparts):
    _check(kernels, shape, "i64sum", nparts)


@pytest.mark.parametrize("nparts", [3, 1000])
@pytest.mark.parametrize("shape", ["cap65536", "sentinel"])
@pytest.mark.parametrize("values", ["i32min_f64max", "f32sum_i64sum"])
def test_value_sets(kernels, values, shape, nparts):
    _check(kernels, shape, values, nparts)


def test_unaligned_table(kernels):
    """A table whose keys start 8 bytes off a 16-byte boundary takes the
    one-slot loads."""
    tkeys, tabs, flags = _table("sentinel", "i64sum")
    odd = torch.empty(tkeys.shape[0] + 1, dtype=torch.int64,
                      device=DEV)[1:]
    odd.copy_(tkeys)
    assert odd.data_ptr() % 16 == 8
    got, gh = kernels._C.groupby_compact_partition(odd, tabs, flags, 8)
    want, wh = kernels._C.groupby_compact_partition(tkeys, tabs, flags, 8)
    assert gh.tolist() == wh.tolist()
    for g, w in zip(_by_partition(got, gh.tolist()[:8]),
                    _by_partition(want, wh.tolist()[:8])):
        assert all(torch.equal(a, b) for a, b in zip(g, w))


def test_finish_partitioned_regrows(kernels):
    """cap_hint 1024 under 5,000 keys: overflow, regrow, retry."""
    g = torch.Generator().manual_seed(11)
    keys = torch.randint(0, 5000, (30000,), generator=g) * 1000003 - 17
    vals = torch.randint(-9, 9, (30000,), generator=g)
    t = kernels.GroupTable([torch.int64], ["sum"], DEV, cap_hint=1024)
    t._mode = "global"  # no sample: straight into the hinted table
    t.insert(keys.to(DEV), [vals.to(DEV)])
    assert t.cap == 1024
    parts = t.finish_partitioned(8)
    assert t.cap > 1024 and len(parts) == 8
    gk = torch.cat([p[0] for p in parts]).cpu()
    gv = torch.cat([p[1][0] for p in parts]).cpu()
    uk, inv = torch.unique(keys, return_inverse=True)
    want = torch.zeros(uk.shape[0], dtype=torch.int64).index_add_(
        0, inv, vals)
    o = torch.argsort(gk)
    assert torch.equal(gk[o], uk) and torch.equal(gv[o], want)


def _reduce(monkeypatch, switch, machine_combiners):
    import bigslice_amd as bs
    monkeypatch.setenv("BIGSLICE_GB_FINISH_PART", switch)
    nshard, rows, nkeys = 8, 25000, 5000

    def data(shard):
        g = torch.Generator().manual_seed(100 + shard)
        return (torch.randint(0, nkeys, (rows,), generator=g) * 7919,
                torch.randint(-100, 100, (rows,), generator=g))

    def build(n):
        def gen(shard, ctx):
            k, v = data(shard)
            yield (k.to(DEV), v.to(DEV))
        return bs.Reduce(bs.ReaderFunc(n, gen, bs.schema_of(int, int)),
                         "sum")

    sess = bs.start(parallelism=4, device=DEV,
                    machine_combiners=machine_combiners)
    try:
        res = sess.run(bs.func(build), nshard)
        gk, gv = [], []
        for f in res.open():
            gk.append(f.columns[0].cpu())
            gv.append(f.columns[1].cpu())
        res.discard()
    finally:
        sess.shutdown()
    gk, gv = torch.cat(gk), torch.cat(gv)
    o = torch.argsort(gk)
    ks, vs = zip(*(data(s) for s in range(nshard)))
    uk, inv = torch.unique(torch.cat(ks), return_inverse=True)
    want = torch.zeros(uk.shape[0], dtype=torch.int64).index_add_(
        0, inv, torch.cat(vs))
    assert torch.equal(gk[o], uk) and torch.equal(gv[o], want)


@pytest.mark.parametrize("machine_combiners", [True, False])
@pytest.mark.parametrize("switch", ["1", "0"])
def test_reduce_end_to_end(kernels, monkeypatch, switch, machine_combiners):
    _reduce(monkeypatch, switch, machine_combiners)
