"""Cardinality sample of GroupTable as one counting kernel.

_C.groupby_sample_distinct(keys, rows) returns a device scalar holding the
number of distinct keys in keys[:rows], minus one: the number the sorted
prefix gave (key changes), so choose_mode sees the same count and the table
layout does not move.  Oracle: torch.unique on the CPU; the count is exact.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I64 = torch.iinfo(torch.int64)


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


@pytest.fixture(scope="module")
def batch():
    """20,001 rows over 5,000 keys, with an element in front so that
    batch[1:] starts 8 bytes off a 16-byte boundary."""
    g = torch.Generator().manual_seed(7)
    return torch.randint(0, 5000, (20002,), dtype=torch.int64, generator=g)


def _check(kernels, keys_dev, rows):
    got = kernels._C.groupby_sample_distinct(keys_dev, rows)
    assert got.dtype == torch.int64 and got.numel() == 1 and got.is_cuda
    want = torch.unique(keys_dev[:rows].cpu()).numel()
    assert int(got.item()) + 1 == want


def test_all_distinct_full_prefix(kernels):
    # 2^19 distinct keys in 2^20 slots: load 0.5, the worst case
    g = torch.Generator().manual_seed(1)
    keys = torch.randperm(1 << 21, generator=g)[:1 << 19] * 2654435761 - 5
    assert torch.unique(keys).numel() == 1 << 19
    _check(kernels, keys.to(DEV), 1 << 19)


def test_one_row(kernels):
    _check(kernels, torch.tensor([42], device=DEV), 1)


def test_255_rows_one_key(kernels):
    _check(kernels, torch.full((255,), -7, dtype=torch.int64, device=DEV),
           255)


def test_prefix_of_a_batch(kernels, batch):
    keys = batch[:20001].to(DEV)
    assert keys.data_ptr() % 16 == 0
    _check(kernels, keys, 4096)
    _check(kernels, keys, 20001)


def test_unaligned_batch(kernels, batch):
    keys = batch.to(DEV)[1:]
    assert keys.data_ptr() % 16 == 8 and keys.shape[0] == 20001
    _check(kernels, keys, 4096)
    _check(kernels, keys, 20001)


def test_extreme_keys(kernels, batch):
    keys = batch[:20001].clone()
    keys[::97] = 0
    keys[1::101] = -1
    keys[2::103] = I64.min + 1
    keys[3::107] = I64.max
    _check(kernels, keys.to(DEV), 20001)


def test_sentinel_rows_among_others(kernels, batch):
    keys = batch[:20001].clone()
    keys[torch.arange(37) * 311 + 5] = kernels.GB_SENTINEL
    assert int((keys == kernels.GB_SENTINEL).sum()) == 37
    _check(kernels, keys.to(DEV), 20001)
    _check(kernels, keys.to(DEV)[1:], 20000)


def test_only_sentinel_prefix(kernels, batch):
    keys = batch[:20001].clone()
    keys[:4096] = kernels.GB_SENTINEL
    _check(kernels, keys.to(DEV), 4096)
    _check(kernels, keys.to(DEV), 1)


def _table_state(kernels, monkeypatch, sample, keys, vals, val_dtype, agg):
    monkeypatch.setenv("BIGSLICE_GB_SAMPLE", sample)
    monkeypatch.setenv("BIGSLICE_GB_SAMPLE_ROWS", "4096")
    t = kernels.GroupTable([val_dtype], [agg], DEV)
    assert t.opts.sample == sample and t.opts.sample_rows == 4096
    half = keys.shape[0] // 2
    t.insert(keys[:half], [vals[:half]])
    t.insert(keys[half:], [vals[half:]])
    k, v = t.finish()
    o = torch.argsort(k)
    return (t._mode, t.cap_hint, t._key_estimate), k[o].cpu(), v[0][o].cpu()


# 40,000 rows (small batches: the sample runs at finish, over the first
# 4,096 rows): 100 keys -> "lds"; 3,000 keys, ~13 rows per key -> "part";
# 40,000 keys, every sampled row its own key -> "sort"
@pytest.mark.parametrize("nkeys,mode", [(100, "lds"), (3000, "part"),
                                        (40000, "sort")])
def test_group_table_same_plan(kernels, monkeypatch, nkeys, mode):
    n = 40000
    g = torch.Generator().manual_seed(nkeys)
    if nkeys == n:
        keys = torch.randperm(n, generator=g) * 7919
    else:
        keys = torch.randint(0, nkeys, (n,), dtype=torch.int64, generator=g)
    vals = torch.randint(-50, 50, (n,), dtype=torch.int64, generator=g)
    keys, vals = keys.to(DEV), vals.to(DEV)
    hs, hk, hv = _table_state(kernels, monkeypatch, "hash", keys, vals,
                              torch.int64, "sum")
    ss, sk, sv = _table_state(kernels, monkeypatch, "sort", keys, vals,
                              torch.int64, "sum")
    assert hs == ss
    assert hs[0] == mode
    assert torch.equal(hk, sk) and torch.equal(hv, sv)
