"""Device hash group-by for multi-column integer keys (K21).

Oracle: torch.unique over the stacked key columns (dim=0) plus a CPU
scatter, never the code under test.  Integer results are exact in any
order (int64 sums wrap modulo 2^64 on both sides) and the float inputs
are small integers, so every summation order gives the same float;
results compare with torch.equal after a lexicographic sort."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1

_SCATTER = {"sum": "sum", "min": "amin", "max": "amax", "prod": "prod"}


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


@pytest.fixture(scope="module")
def gbm(kernels):
    from bigslice_amd.kernels import groupby_multi
    return groupby_multi


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    monkeypatch.delenv("BIGSLICE_GB_FP_BITS", raising=False)
    monkeypatch.delenv("BIGSLICE_GB_MULTIKEY", raising=False)


def _vals(n, seed):
    """Small values of both signs, every third row near +-2^62 so the
    per-key sums wrap (as in the K19 tests)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-1000, 1000, (n,), dtype=torch.int64, generator=g)
    big = (1 << 62) - torch.randint(0, 1000, (n,), dtype=torch.int64,
                                    generator=g)
    sign = torch.randint(0, 2, (n,), dtype=torch.int64, generator=g) * 2 - 1
    third = torch.arange(n) % 3 == 0
    return torch.where(third, sign * big, v)


def _lexsort(keys, vals):
    """Rows ordered by the key columns, first column most significant."""
    perm = torch.arange(keys[0].shape[0])
    for kc in reversed(keys):
        perm = perm[torch.sort(kc[perm], stable=True).indices]
    return [k[perm] for k in keys], [v[perm] for v in vals]


def _oracle(batches, aggs):
    """batches: [(key columns, value columns)] on the CPU."""
    keys = [torch.cat(c) for c in zip(*(k for k, _ in batches))]
    vals = [torch.cat(c) for c in zip(*(v for _, v in batches))]
    stacked = torch.stack([k.to(torch.int64) for k in keys], 1)
    uk, inv = torch.unique(stacked, dim=0, return_inverse=True)
    outs = []
    for v, a in zip(vals, aggs):
        out = torch.empty(uk.shape[0], dtype=v.dtype)
        outs.append(out.scatter_reduce_(0, inv, v, reduce=_SCATTER[a],
                                        include_self=False))
    ukeys = [uk[:, c].to(keys[c].dtype) for c in range(len(keys))]
    return _lexsort(ukeys, outs)


def _fallback():
    from bigslice_amd.ops.aggregate import Aggregation, _combine_once

    def make(aggs):
        return lambda k, v: _combine_once(k, v, Aggregation(aggs))
    return make


def _run(gbm, batches, aggs, cap_hint=None):
    """The batches through one MultiKeyTable; returns (sorted key columns,
    sorted value columns) on the CPU, and the table."""
    nkey = len(batches[0][0])
    t = gbm.MultiKeyTable(nkey, [v.dtype for v in batches[0][1]], aggs,
                          DEV, cap_hint=cap_hint,
                          fallback=_fallback()(aggs))
    for k, v in batches:
        t.insert([c.to(DEV) for c in k], [c.to(DEV) for c in v])
    gk, gv = t.finish()
    gk, gv = _lexsort([c.cpu() for c in gk], [c.cpu() for c in gv])
    return gk, gv, t


def _check(gbm, batches, aggs=("sum",), cap_hint=None):
    aggs = list(aggs)
    wk, wv = _oracle(batches, aggs)
    gk, gv, t = _run(gbm, batches, aggs, cap_hint)
    assert len(gk) == len(wk) and len(gv) == len(wv)
    for g, w in zip(gk + gv, wk + wv):
        assert g.dtype == w.dtype
        assert torch.equal(g, w)
    return t


def _fallbacks():
    from bigslice_amd.utils import stats
    return stats.DEFAULT.values().get("combiner/fingerprint_fallbacks", 0)


def _rand_keys(n, ncols, card, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-card, card, (n,), dtype=torch.int64, generator=g)
            for _ in range(ncols)]


@pytest.mark.parametrize("ncols", [2, 3, 8])
def test_device_fingerprint_is_the_mirror(kernels, gbm, ncols):
    g = torch.Generator().manual_seed(ncols)
    n = 70_000
    cols = [torch.randint(INT64_MIN, INT64_MAX, (n,), dtype=torch.int64,
                          generator=g) for _ in range(ncols)]
    edge = torch.tensor([0, -1, INT64_MIN, INT64_MAX], dtype=torch.int64)
    for c in range(ncols):
        cols[c][:4] = edge.roll(c)
    dev = [c.to(DEV) for c in cols]
    for bits in (64, 4):
        got = kernels._C.groupby_mk_fingerprint(dev, bits).cpu()
        assert torch.equal(got, gbm.fingerprint64(cols, bits))


@pytest.mark.parametrize("n", [1, 257, 70_000])
@pytest.mark.parametrize("ncols", [2, 3, 5])
def test_row_counts(gbm, n, ncols):
    keys = _rand_keys(n, ncols, 6, seed=n + ncols)
    _check(gbm, [(keys, [_vals(n, n)])])


@pytest.mark.parametrize("ncols", [2, 3, 4, 8])
def test_tuples_differing_in_one_column(gbm, ncols):
    """A base tuple and, per position, tuples that differ from it there
    only; every one 37 times."""
    base = torch.arange(100, 100 + ncols, dtype=torch.int64)
    rows = [base]
    for c in range(ncols):
        for delta in (1, -1, 1 << 40):
            r = base.clone()
            r[c] += delta
            rows.append(r)
    tuples = torch.stack(rows).repeat(37, 1)
    tuples = tuples[torch.randperm(tuples.shape[0],
                                   generator=torch.Generator().manual_seed(0))]
    keys = [tuples[:, c].contiguous() for c in range(ncols)]
    n = tuples.shape[0]
    t = _check(gbm, [(keys, [_vals(n, 7)])])
    assert t.rows == n


def test_swapped_pairs(gbm):
    g = torch.Generator().manual_seed(3)
    a = torch.randint(-50, 50, (5000,), dtype=torch.int64, generator=g)
    b = torch.randint(-50, 50, (5000,), dtype=torch.int64, generator=g)
    keys = [torch.cat([a, b, a, b]), torch.cat([b, a, a, b])]
    _check(gbm, [(keys, [_vals(20_000, 3)])])


@pytest.mark.parametrize("ncols", [2, 3])
def test_extreme_key_values_in_every_column(gbm, ncols):
    """INT64_MIN is the value of the tag array's empty marker; as a key
    value it is as good as any."""
    import itertools
    edge = [INT64_MIN, 0, -1, INT64_MAX]
    tuples = torch.tensor(list(itertools.product(edge, repeat=ncols)),
                          dtype=torch.int64).repeat(5, 1)
    keys = [tuples[:, c].contiguous() for c in range(ncols)]
    _check(gbm, [(keys, [_vals(tuples.shape[0], 11)])])


def test_one_tuple_many_rows(gbm):
    n = 4096
    keys = [torch.full((n,), 42, dtype=torch.int64),
            torch.full((n,), -42, dtype=torch.int64)]
    t = _check(gbm, [(keys, [_vals(n, 5)])])
    gk, gv, _ = _run(gbm, [(keys, [torch.ones(n, dtype=torch.int64)])],
                     ["sum"])
    assert gv[0].tolist() == [n]


def test_overflow_regrows_and_reinserts(gbm):
    n = 5000
    keys = [torch.arange(n, dtype=torch.int64) // 70,
            torch.arange(n, dtype=torch.int64) % 70]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(9))
    keys = [k[perm] for k in keys]
    before = _fallbacks()
    t = _check(gbm, [(keys, [_vals(n, 9)])], cap_hint=1024)
    assert t.cap > 1024
    assert _fallbacks() == before


def test_batches_repeat_and_add_tuples(gbm):
    batches = []
    for b in range(3):
        n = 3000 + 17 * b
        g = torch.Generator().manual_seed(20 + b)
        # the tuple space grows with every batch and contains the last
        keys = [torch.randint(0, 20 * (b + 1), (n,), dtype=torch.int64,
                              generator=g),
                torch.randint(-3, 4, (n,), dtype=torch.int64, generator=g)]
        batches.append((keys, [_vals(n, 30 + b)]))
    _check(gbm, batches)


def test_value_dtypes_and_aggregations(gbm):
    n = 20_000
    g = torch.Generator().manual_seed(77)
    keys = _rand_keys(n, 3, 4, seed=77)
    # at most ~60 rows per tuple have a 2: the product stays below 2^63
    prod = torch.where(torch.arange(n) % 9 == 0,
                       torch.full((n,), 2, dtype=torch.int64),
                       torch.randint(0, 2, (n,), dtype=torch.int64,
                                     generator=g) * 2 - 1)
    vals = [
        _vals(n, 77),
        torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int64,
                      generator=g).to(torch.int32),
        torch.randint(-1000, 1000, (n,), dtype=torch.int64,
                      generator=g).to(torch.float64),
        prod,
        torch.randint(-8, 9, (n,), dtype=torch.int64,
                      generator=g).to(torch.float32),
    ]
    _check(gbm, [(keys, vals)], aggs=["sum", "min", "max", "prod", "sum"])


def test_int32_key_column_comes_back_int32(gbm):
    n = 10_000
    g = torch.Generator().manual_seed(4)
    keys = [torch.randint(-(1 << 31), (1 << 31) - 1, (n,),
                          dtype=torch.int64, generator=g).to(torch.int32)
            % 13,
            torch.randint(-5, 5, (n,), dtype=torch.int64, generator=g)]
    keys[0][:3] = torch.tensor([-(1 << 31), (1 << 31) - 1, -1],
                               dtype=torch.int32)
    wk, _ = _oracle([(keys, [_vals(n, 4)])], ["sum"])
    assert wk[0].dtype == torch.int32
    _check(gbm, [(keys, [_vals(n, 4)])])


def test_narrow_fingerprint_falls_back_exactly(gbm, monkeypatch):
    """64 distinct tuples cannot have 64 different 4-bit tags."""
    monkeypatch.setenv("BIGSLICE_GB_FP_BITS", "4")
    n = 6400
    keys = [torch.arange(n, dtype=torch.int64) % 8,
            (torch.arange(n, dtype=torch.int64) // 8) % 8]
    before = _fallbacks()
    t = _check(gbm, [(keys, [_vals(n, 1)])])
    assert t.opts.fp_bits == 4
    assert _fallbacks() == before + 1


def test_narrow_fingerprint_one_tuple_needs_no_fallback(gbm, monkeypatch):
    monkeypatch.setenv("BIGSLICE_GB_FP_BITS", "4")
    n = 1000
    keys = [torch.full((n,), 7, dtype=torch.int64),
            torch.full((n,), INT64_MIN, dtype=torch.int64)]
    before = _fallbacks()
    t = _check(gbm, [(keys, [_vals(n, 2)])])
    assert t.opts.fp_bits == 4
    assert _fallbacks() == before


def _reduce_rows(device):
    import bigslice_amd as bs
    g = torch.Generator().manual_seed(8)
    n = 50_000
    k1 = torch.randint(0, 40, (n,), dtype=torch.int64, generator=g)
    k2 = torch.randint(-20, 20, (n,), dtype=torch.int64, generator=g)
    v = _vals(n, 8)

    def job():
        return bs.Reduce(bs.Prefixed(bs.Const(4, k1, k2, v), 2), "sum")
    sess = bs.start(parallelism=2, device=device)
    rows = sorted(tuple(int(x) for x in r)
                  for r in sess.run(bs.func(job)).scan())
    sess.shutdown()
    return rows


def test_reduce_over_a_two_column_prefix(kernels, monkeypatch):
    calls = []
    real = kernels._C.groupby_mk_insert

    def spy(*a, **kw):
        calls.append(a[0][0].shape[0])
        return real(*a, **kw)
    monkeypatch.setattr(kernels._C, "groupby_mk_insert", spy)
    want = _reduce_rows("cpu")
    assert calls == []
    got = _reduce_rows(DEV)
    assert calls, "the multi-column table did not run"
    assert got == want
    ran = len(calls)
    monkeypatch.setenv("BIGSLICE_GB_MULTIKEY", "0")
    assert _reduce_rows(DEV) == want
    assert len(calls) == ran
