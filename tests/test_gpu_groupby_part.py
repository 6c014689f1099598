"""Partitioned LDS pre-aggregating group-by insert (K19, mode "part").

Oracle: the same rows through GroupTable with BIGSLICE_GB_MODE=global and
through a CPU torch.unique + scatter_add.  int64 sums are exact in any
order (they wrap modulo 2^64 in both), so results compare with
torch.equal after ordering by key."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


@pytest.fixture(scope="module")
def T(kernels):
    return kernels.PART_TILE_ROWS


def _vals(n, seed):
    """Small values of both signs, every third row near +-2^62 so the
    per-key sums wrap."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-1000, 1000, (n,), dtype=torch.int64, generator=g)
    big = (1 << 62) - torch.randint(0, 1000, (n,), dtype=torch.int64,
                                    generator=g)
    sign = torch.randint(0, 2, (n,), dtype=torch.int64, generator=g) * 2 - 1
    third = torch.arange(n) % 3 == 0
    return torch.where(third, sign * big, v)


def _cpu_oracle(batches):
    keys = torch.cat([k for k, _ in batches])
    vals = torch.cat([v for _, v in batches])
    uk, inv = torch.unique(keys, return_inverse=True)
    sums = torch.zeros(uk.shape[0], dtype=torch.int64).scatter_add_(
        0, inv, vals)
    return uk, sums


def _run(kernels, monkeypatch, mode, batches, min_rows=1, cap_hint=None):
    """Feed CPU batches through one GroupTable in the forced mode; returns
    (keys, sums) ordered by key, the table, and how often the
    partitioned insert ran."""
    monkeypatch.setenv("BIGSLICE_GB_MODE", mode)
    monkeypatch.setattr(kernels.GroupTable, "_PART_MIN_ROWS", min_rows)
    calls = []
    real = kernels._C.groupby_insert_part

    def spy(*a):
        calls.append(a[0].shape[0])
        return real(*a)
    monkeypatch.setattr(kernels._C, "groupby_insert_part", spy)
    t = kernels.GroupTable([torch.int64], ["sum"], DEV, cap_hint=cap_hint)
    for k, v in batches:
        t.insert(k.to(DEV), [v.to(DEV)])
    uk, outs = t.finish()
    order = torch.argsort(uk)
    return uk[order].cpu(), outs[0][order].cpu(), t, calls


def _check(kernels, monkeypatch, batches, part_calls, **kw):
    want_k, want_s = _cpu_oracle(batches)
    gk, gs, _, calls = _run(kernels, monkeypatch, "global", batches, **kw)
    assert calls == []
    assert torch.equal(gk, want_k) and torch.equal(gs, want_s)
    pk, ps, table, calls = _run(kernels, monkeypatch, "part", batches, **kw)
    assert len(calls) == part_calls, calls
    assert torch.equal(pk, want_k)
    assert torch.equal(ps, want_s)
    return table


@pytest.mark.parametrize("which", ["1", "63", "65", "T-1", "T", "T+1",
                                   "3T+17"])
def test_row_counts_uniform_keys(kernels, monkeypatch, T, which):
    n = {"1": 1, "63": 63, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1,
         "3T+17": 3 * T + 17}[which]
    g = torch.Generator().manual_seed(n)
    keys = torch.randint(0, 1000, (n,), dtype=torch.int64, generator=g)
    _check(kernels, monkeypatch, [(keys, _vals(n, n))], 1)


def test_one_key(kernels, monkeypatch, T):
    # same-address LDS atomics; one bucket spanning every tile
    n = 3 * T + 17
    keys = torch.full((n,), 424242, dtype=torch.int64)
    _check(kernels, monkeypatch, [(keys, _vals(n, 1))], 1)


def test_all_distinct(kernels, monkeypatch, T):
    # more distinct keys per tile than LDS slots: the probe chain runs
    # out and rows fall through to the global insert
    n = 4 * T
    assert T > kernels.PART_LDS_SLOTS // 2
    g = torch.Generator().manual_seed(2)
    keys = torch.randperm(n, generator=g) * 7919 - 1000
    _check(kernels, monkeypatch, [(keys, _vals(n, 2))], 1)


def test_negative_keys(kernels, monkeypatch, T):
    n = 3 * T + 17
    g = torch.Generator().manual_seed(3)
    keys = -torch.randint(1, 5000, (n,), dtype=torch.int64, generator=g)
    keys[::5] = -(1 << 63) + 1 + keys[::5] * -1  # near the sentinel
    _check(kernels, monkeypatch, [(keys, _vals(n, 3))], 1)


def test_sentinel_keys(kernels, monkeypatch, T):
    n = 3 * T + 17
    g = torch.Generator().manual_seed(4)
    keys = torch.randint(0, 1000, (n,), dtype=torch.int64, generator=g)
    keys[::11] = kernels.GB_SENTINEL
    vals = _vals(n, 4)
    table = _check(kernels, monkeypatch, [(keys, vals)], 1)
    assert int(table.flags[0].item()) == 1  # sentinel_seen
    want = vals[::11].sum()  # wraps like the table's adds
    assert int(table.tabs[0][table.cap].item()) == int(want)


def test_no_sentinel_flag_without_sentinel_rows(kernels, monkeypatch, T):
    n = T + 1
    keys = torch.arange(n, dtype=torch.int64) % 300
    table = _check(kernels, monkeypatch, [(keys, _vals(n, 5))], 1)
    assert int(table.flags[0].item()) == 0


def test_streaming_mixed_batches(kernels, monkeypatch, T):
    # large batches take the partitioned path, small ones the plain
    # insert, all into one table, overlapping key sets, one finish()
    g = torch.Generator().manual_seed(6)
    batches = []
    for i, n in enumerate([3 * T + 17, 1000, 2 * T, 999, T]):
        keys = torch.randint(100 * i, 100 * i + 2000, (n,),
                             dtype=torch.int64, generator=g)
        batches.append((keys, _vals(n, 10 + i)))
    _check(kernels, monkeypatch, batches, 3, min_rows=T)


def test_regrow(kernels, monkeypatch):
    # 100k distinct keys into a 1024-slot table: overflow flag, regrow,
    # re-insert of the retained (unpartitioned) batches
    g = torch.Generator().manual_seed(7)
    keys = torch.cat([torch.randperm(100_000, generator=g),
                      torch.randperm(100_000, generator=g)]) * 31 - 5
    batches = [(keys, _vals(keys.shape[0], 7))]
    want_k, want_s = _cpu_oracle(batches)
    pk, ps, table, calls = _run(kernels, monkeypatch, "part", batches,
                                cap_hint=1024)
    assert len(calls) >= 2, calls  # first insert + re-insert after regrow
    assert table.cap > 1024
    assert torch.equal(pk, want_k) and torch.equal(ps, want_s)


def _lex_sorted(k, v):
    o = torch.argsort(v, stable=True)
    o = o[torch.argsort(k[o], stable=True)]
    return k[o], v[o]


@pytest.mark.parametrize("which", ["T-1", "T+1", "3T+17"])
@pytest.mark.parametrize("big", [False, True])
def test_scatter_alone(kernels, T, which, big):
    n = {"T-1": T - 1, "T+1": T + 1, "3T+17": 3 * T + 17}[which]
    B = kernels.PART_MAX_BUCKETS if big else 2
    cap = 1 << 20
    g = torch.Generator().manual_seed(n + B)
    keys = torch.randint(-2**62, 2**62, (n,), dtype=torch.int64,
                         generator=g)
    keys[::97] = kernels.GB_SENTINEL
    keys[1::2] = keys[0::2][: keys[1::2].shape[0]]  # duplicates too
    vals = _vals(n, B)
    pairs, totals = kernels._C.groupby_part_scatter(
        keys.to(DEV), vals.to(DEV), cap, B)
    assert pairs.shape == (n, 2) and totals.shape == (B,)
    ok = pairs[:, 0].contiguous()
    # a permutation of the input pairs
    gk, gv = _lex_sorted(ok.cpu(), pairs[:, 1].cpu())
    wk, wv = _lex_sorted(keys, vals)
    assert torch.equal(gk, wk) and torch.equal(gv, wv)
    # bucket ids (sentinel rows: bucket 0) never decrease along the output
    bids = kernels._C.slot_pids(ok, cap, B).cpu().to(torch.int64)
    bids[ok.cpu() == kernels.GB_SENTINEL] = 0
    assert bool((bids[1:] >= bids[:-1]).all())
    # per-bucket counts
    totals = totals.cpu().to(torch.int64)
    assert int(totals.sum()) == n
    assert torch.equal(torch.bincount(bids, minlength=B), totals)
