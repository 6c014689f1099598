"""Tile groups of the partitioned group-by insert (K19).

The histogram and the scatter run one workgroup per group of G consecutive
4096-row tiles; the workgroup carries each bucket's cursor from tile to
tile.  G is forced here through the trailing `group_tiles` argument and
through BIGSLICE_GB_PART_GROUP.  Oracles: the input itself (the scatter
permutes it), _C.slot_pids for the bucket of a key, and CPU torch.unique +
scatter_add for the sums, which are int64 and compare exactly."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R = 4096  # rows of a scatter tile
CAP = 1 << 20


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    assert k._C.GBP_SCATTER_ROWS == R
    return k


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


def _lex_sorted(k, v):
    o = torch.argsort(v, stable=True)
    o = o[torch.argsort(k[o], stable=True)]
    return k[o], v[o]


def _bucket_ids(kernels, keys_dev, B):
    """Bucket of every key (sentinel rows: bucket 0), on the CPU."""
    bids = kernels._C.slot_pids(keys_dev, CAP, B).cpu().to(torch.int64)
    bids[keys_dev.cpu() == kernels.GB_SENTINEL] = 0
    return bids


def _to_dev(x, odd):
    """x on the device; odd: at an address that is 8 mod 16 (the kernels
    load two rows at once only from 16-byte aligned columns)."""
    if not odd:
        return x.to(DEV)
    y = torch.empty(x.shape[0] + 1, dtype=x.dtype, device=DEV)[1:]
    y.copy_(x)
    assert y.data_ptr() % 16 == 8 and y.is_contiguous()
    return y


def _check_scatter(kernels, keys, vals, B, G, odd=(False, False)):
    n = keys.shape[0]
    dk = _to_dev(keys, odd[0])
    pairs, totals = kernels._C.groupby_part_scatter(
        dk, _to_dev(vals, odd[1]), CAP, B, G)
    assert pairs.shape == (n, 2) and totals.shape == (B,)
    ok = pairs[:, 0].contiguous()
    # a permutation of the input pairs
    gk, gv = _lex_sorted(ok.cpu(), pairs[:, 1].cpu())
    wk, wv = _lex_sorted(keys, vals)
    assert torch.equal(gk, wk) and torch.equal(gv, wv)
    # bucket ids never decrease along the output
    bids = _bucket_ids(kernels, ok, B)
    assert bool((bids[1:] >= bids[:-1]).all())
    # per-bucket counts: exactly those of the input
    totals = totals.cpu().to(torch.int64)
    assert int(totals.sum()) == n
    want = torch.bincount(_bucket_ids(kernels, dk, B), minlength=B)
    assert torch.equal(totals, want)
    assert torch.equal(torch.bincount(bids, minlength=B), totals)
    return totals


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("which", ["R-1", "GR-1", "GR", "GR+1", "2GR+17"])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_scatter_alone(kernels, G, which, big):
    n = {"R-1": R - 1, "GR-1": G * R - 1, "GR": G * R, "GR+1": G * R + 1,
         "2GR+17": 2 * G * R + 17}[which]
    B = kernels.PART_MAX_BUCKETS if big else 2
    g = torch.Generator().manual_seed(n + B)
    keys = torch.randint(-2**62, 2**62, (n,), dtype=torch.int64,
                         generator=g)
    keys[::97] = kernels.GB_SENTINEL
    keys[1::2] = keys[0::2][: keys[1::2].shape[0]]  # duplicates too
    _check_scatter(kernels, keys, _vals(n, B), B, G)


@pytest.mark.parametrize("odd", [(True, True), (True, False),
                                 (False, True)])
@pytest.mark.parametrize("n", [R + 1, 2 * 4 * R + 17])
def test_scatter_unaligned_columns(kernels, n, odd):
    # a column that is not 16-byte aligned takes the one-row loads
    B = kernels.PART_MAX_BUCKETS
    g = torch.Generator().manual_seed(n)
    keys = torch.randint(-2**62, 2**62, (n,), dtype=torch.int64,
                         generator=g)
    keys[::97] = kernels.GB_SENTINEL
    _check_scatter(kernels, keys, _vals(n, 7), B, 4, odd)


def test_one_bucket_spans_everything(kernels):
    # the cursor of one bucket carried across every tile and every group
    G, B = 4, kernels.PART_MAX_BUCKETS
    n = 2 * G * R + 17
    keys = torch.full((n,), 424242, dtype=torch.int64)
    totals = _check_scatter(kernels, keys, _vals(n, 1), B, G)
    b = int(_bucket_ids(kernels, keys[:1].to(DEV), B)[0])
    want = torch.zeros(B, dtype=torch.int64)
    want[b] = n
    assert torch.equal(totals, want)


@pytest.mark.parametrize("n,want", [(1 << 21, 1), (7_812_500, 4),
                                    (8_388_608, 4), ((1 << 31) - 1, 8)])
def test_group_rule(kernels, n, want):
    # smallest G that leaves at most two workgroups per CU (512), capped
    # at 8
    assert kernels._C.groupby_part_group_tiles(n) == want


@pytest.fixture(scope="module")
def e2e_batches():
    sizes = [2 * 4 * R + 17, R + 1, 4 * R]
    g = torch.Generator().manual_seed(21)
    batches = []
    for i, n in enumerate(sizes):
        keys = torch.randint(1000 * i, 1000 * i + 3000, (n,),
                             dtype=torch.int64, generator=g)
        batches.append((keys, _vals(n, 30 + i)))
    keys = torch.cat([k for k, _ in batches])
    vals = torch.cat([v for _, v in batches])
    uk, inv = torch.unique(keys, return_inverse=True)
    sums = torch.zeros(uk.shape[0], dtype=torch.int64).scatter_add_(
        0, inv, vals)
    return batches, uk, sums


@pytest.mark.parametrize("owned", ["0", "1"])
@pytest.mark.parametrize("group", ["1", "4"])
def test_end_to_end(kernels, monkeypatch, e2e_batches, group, owned):
    batches, want_k, want_s = e2e_batches
    monkeypatch.setenv("BIGSLICE_GB_MODE", "part")
    monkeypatch.setenv("BIGSLICE_GB_PART_GROUP", group)
    monkeypatch.setenv("BIGSLICE_GB_PART_OWNED", owned)
    monkeypatch.setattr(kernels.GroupTable, "_PART_MIN_ROWS", 1)
    calls = []
    real = kernels._C.groupby_insert_part

    def spy(*a):
        calls.append(a[7:])
        return real(*a)
    monkeypatch.setattr(kernels._C, "groupby_insert_part", spy)
    t = kernels.GroupTable([torch.int64], ["sum"], DEV)
    for k, v in batches:
        t.insert(k.to(DEV), [v.to(DEV)])
    uk, outs = t.finish()
    # every batch took the partitioned insert, in the asked variant
    assert calls == [(int(owned), int(group))] * len(batches), calls
    order = torch.argsort(uk)
    assert torch.equal(uk[order].cpu(), want_k)
    assert torch.equal(outs[0][order].cpu(), want_s)
