"""Bucket-owning aggregate pass of the partitioned group-by insert (K19).

A workgroup loads the table slice of its bucket into LDS, probes it there
and stores it back; what it cannot place is left, per bucket, as
clean[b] rows at the front of the bucket's segment for the tiled cleanup
pass.  Oracle as in test_gpu_groupby_part.py: CPU torch.unique +
scatter_add_ and the same rows through BIGSLICE_GB_MODE=global, compared
with torch.equal after ordering by key (int64 sums wrap alike in any
order).  Every case runs with the owned pass on and off."""

import pytest
import torch

gpu = pytest.mark.gpu

DEV = "cuda:0"

both = pytest.mark.parametrize("owned", ["1", "0"])


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


def _run(kernels, monkeypatch, mode, owned, batches, min_rows=1,
         cap_hint=None):
    """Feed CPU batches through one GroupTable in the forced mode; returns
    (keys, sums) ordered by key, the table, and the `owned` argument of
    every partitioned insert that ran."""
    monkeypatch.setenv("BIGSLICE_GB_MODE", mode)
    monkeypatch.setenv("BIGSLICE_GB_PART_OWNED", owned)
    monkeypatch.setattr(kernels.GroupTable, "_PART_MIN_ROWS", min_rows)
    calls = []
    real = kernels._C.groupby_insert_part

    def spy(*a):
        calls.append(a[7] if len(a) > 7 else 0)
        return real(*a)
    monkeypatch.setattr(kernels._C, "groupby_insert_part", spy)
    t = kernels.GroupTable([torch.int64], ["sum"], DEV, cap_hint=cap_hint)
    for k, v in batches:
        t.insert(k.to(DEV), [v.to(DEV)])
    uk, outs = t.finish()
    order = torch.argsort(uk)
    return uk[order].cpu(), outs[0][order].cpu(), t, calls


def _check(kernels, monkeypatch, owned, batches, part_calls, **kw):
    want_k, want_s = _cpu_oracle(batches)
    gk, gs, _, calls = _run(kernels, monkeypatch, "global", owned, batches,
                            **kw)
    assert calls == []
    assert torch.equal(gk, want_k) and torch.equal(gs, want_s)
    pk, ps, table, calls = _run(kernels, monkeypatch, "part", owned,
                                batches, **kw)
    if part_calls is not None:
        assert calls == [int(owned)] * part_calls, calls
    else:
        assert calls and all(c == int(owned) for c in calls), calls
    assert torch.equal(pk, want_k)
    assert torch.equal(ps, want_s)
    return table


def _direct(kernels, keys, vals, cap, B, table=None):
    """Scatter, then the owner and cleanup passes alone, into a table of
    cap slots.  Returns (clean, totals, starts, pairs after the passes,
    table)."""
    C = kernels._C
    if table is None:
        table = kernels.GroupTable([torch.int64], ["sum"], DEV)
        table._alloc(cap)
    pairs, totals = C.groupby_part_scatter(keys.to(DEV), vals.to(DEV), cap,
                                           B)
    clean = C.groupby_part_owned(pairs, totals, table.tkeys, table.tabs[0],
                                 table.flags, kernels.MAX_PROBES)
    totals = totals.cpu().to(torch.int64)
    starts = torch.cumsum(totals, 0) - totals
    return clean.cpu().to(torch.int64), totals, starts, pairs.cpu(), table


def _table_result(kernels, table):
    tk = table.tkeys[:table.cap].cpu()
    used = tk != kernels.GB_SENTINEL
    k, s = tk[used], table.tabs[0][:table.cap].cpu()[used]
    o = torch.argsort(k)
    return k[o], s[o]


def _home_slots(kernels, keys, cap):
    """Table slot each key hashes to (bucket id at a fan-out of cap)."""
    return kernels._C.slot_pids(keys.to(DEV), cap, cap).cpu().to(torch.int64)


def _probe(homes, cap, S):
    """Linear probing of distinct keys with the given home slots into an
    empty table of cap slots, on the CPU.  Returns
    * the longest run of taken slots in the full table (circular): no
      probe, in any insertion order, walks further than that;
    * per slice of S slots, how many keys find no slot between their
      home and the end of the slice when only that slice's own keys are
      inserted, which is what the slice's owner sees.
    Both are independent of the insertion order."""
    homes = homes.tolist()
    taken = [False] * cap
    for h in homes:
        while taken[h % cap]:
            h += 1
        taken[h % cap] = True
    worst = run = 0
    for i in range(2 * cap):
        run = run + 1 if taken[i % cap] else 0
        worst = max(worst, min(run, cap))
    own = [False] * cap
    left = [0] * (cap // S)
    for h in homes:
        end = (h // S + 1) * S
        while h < end and own[h]:
            h += 1
        if h < end:
            own[h] = True
        else:
            left[(end - 1) // S] += 1
    return worst, left


# ---------------------------------------------------------------- row counts

@gpu
@both
@pytest.mark.parametrize("which", ["1", "63", "65", "T-1", "T", "T+1",
                                   "3T+17"])
def test_row_counts_uniform_keys(kernels, monkeypatch, T, owned, which):
    n = {"1": 1, "63": 63, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1,
         "3T+17": 3 * T + 17}[which]
    g = torch.Generator().manual_seed(n)
    keys = torch.randint(0, 1000, (n,), dtype=torch.int64, generator=g)
    _check(kernels, monkeypatch, owned, [(keys, _vals(n, n))], 1)


@gpu
@both
def test_fewer_keys_than_buckets(kernels, monkeypatch, T, owned):
    # 8T rows -> at least 8 buckets, 3 keys: most buckets are empty
    n = 8 * T + 5
    keys = torch.arange(n, dtype=torch.int64) % 3 * 1_000_003 - 7
    batches = [(keys, _vals(n, 21))]
    _check(kernels, monkeypatch, owned, batches, 1)
    if owned == "1":
        cap, B = 1 << 14, 8
        clean, totals, _, _, table = _direct(kernels, keys, batches[0][1],
                                             cap, B)
        assert int((totals == 0).sum()) >= B - 3
        # an empty bucket leaves nothing behind; a full one at most what
        # lies beyond the owner's limit
        assert torch.equal(
            clean, (totals - kernels.PART_OWN_LIMIT).clamp(min=0))
        k, s = _table_result(kernels, table)
        want_k, want_s = _cpu_oracle(batches)
        assert torch.equal(k, want_k) and torch.equal(s, want_s)


# ------------------------------------------------- chains that leave a slice

CHAIN_CAP = 1024


@pytest.fixture(scope="module")
def chain_keys(kernels):
    """~700 distinct keys for a 1024-slot table split into two slices of
    512: eight of them hash into the last four slots of each slice, so a
    chain must cross slot 511|512 and another must wrap at 1023|0.  The
    largest displacement stays well under MAX_PROBES, so the table does
    not regrow."""
    cap, S = CHAIN_CAP, CHAIN_CAP // 2
    g = torch.Generator().manual_seed(99)
    pool = torch.unique(torch.randint(-2**62, 2**62, (60000,),
                                      dtype=torch.int64, generator=g))
    pool = pool[torch.randperm(pool.shape[0], generator=g)]
    homes = _home_slots(kernels, pool, cap)
    edge0 = pool[(homes >= S - 4) & (homes < S)][:8]
    edge1 = pool[homes >= cap - 4][:8]
    assert edge0.shape[0] == 8 and edge1.shape[0] == 8
    inner = pool[(homes % S) < S - 4]
    limit = kernels.MAX_PROBES - 8
    for attempt in range(16):
        keys = torch.cat([inner[attempt * 684:(attempt + 1) * 684],
                          edge0, edge1])
        worst, left = _probe(_home_slots(kernels, keys, cap), cap, S)
        if worst <= limit:
            break
    assert worst <= limit, worst
    assert left[0] >= 4 and left[1] >= 4, left
    return keys, left


def _chain_batch(keys, n, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.cat([torch.arange(keys.shape[0]),  # every key at least once
                     torch.randint(0, keys.shape[0], (n - keys.shape[0],),
                                   generator=g)])
    return keys[idx[torch.randperm(n, generator=g)]], _vals(n, seed)


@gpu
@both
def test_chains_leave_slice_and_wrap(kernels, monkeypatch, T, owned,
                                     chain_keys):
    keys, left = chain_keys
    batch = _chain_batch(keys, 2 * T, 31)
    table = _check(kernels, monkeypatch, owned, [batch], 1,
                   cap_hint=CHAIN_CAP)
    assert table.cap == CHAIN_CAP  # B = 2, slices of 512
    if owned == "1":
        clean, totals, starts, pairs, table = _direct(
            kernels, batch[0], batch[1], CHAIN_CAP, 2)
        assert int(totals.max()) <= kernels.PART_OWN_LIMIT
        for b in range(2):
            # all rows were processed: clean counts spilled rows only,
            # and exactly the keys that do not fit before the slice end
            # were spilled
            assert 0 < int(clean[b]) < int(totals[b])
            s = int(starts[b])
            spilled = pairs[s:s + int(clean[b]), 0]
            assert torch.unique(spilled).shape[0] == left[b]
        k, s = _table_result(kernels, table)
        want_k, want_s = _cpu_oracle([batch])
        assert torch.equal(k, want_k) and torch.equal(s, want_s)
        assert int(table.flags[1].item()) == 0  # no overflow


@gpu
@both
def test_key_already_stored_past_slice_end(kernels, monkeypatch, T, owned,
                                           chain_keys):
    # batch 1 (below min_rows) goes through the plain insert and stores
    # some keys beyond the end of their home slice; batch 2 goes through
    # the partitioned insert and has to find them there
    keys, _ = chain_keys
    b1 = _chain_batch(keys, 2 * keys.shape[0], 32)
    b2 = _chain_batch(keys, 2 * T, 33)
    table = _check(kernels, monkeypatch, owned, [b1, b2], 1, min_rows=T,
                   cap_hint=CHAIN_CAP)
    assert table.cap == CHAIN_CAP
    if owned == "1":
        # the same two steps by hand: after the plain insert of batch 1
        # some key does sit in another slice than its home slot's
        S = CHAIN_CAP // 2
        t = kernels.GroupTable([torch.int64], ["sum"], DEV)
        t._alloc(CHAIN_CAP)
        kernels._C.groupby_insert(b1[0].to(DEV), [b1[1].to(DEV)], t.codes,
                                  t.tkeys, t.tabs, t.flags,
                                  kernels.MAX_PROBES)
        tk = t.tkeys[:CHAIN_CAP].cpu()
        slots = torch.nonzero(tk != kernels.GB_SENTINEL).flatten()
        homes = _home_slots(kernels, tk[slots], CHAIN_CAP)
        away = homes // S != slots // S
        assert bool(away[homes < S].any()) and bool(away[homes >= S].any())
        # the owner of either slice has to spill those keys' rows again
        clean, _, starts, pairs, _ = _direct(kernels, b2[0], b2[1],
                                             CHAIN_CAP, 2, table=t)
        for b in range(2):
            s = int(starts[b])
            spilled = torch.unique(pairs[s:s + int(clean[b]), 0])
            stored_away = tk[slots][away & (homes // S == b)]
            assert set(stored_away.tolist()) <= set(spilled.tolist())
        k, s = _table_result(kernels, t)
        want_k, want_s = _cpu_oracle([b1, b2])
        assert torch.equal(k, want_k) and torch.equal(s, want_s)


# ---------------------------------------------------------- oversize buckets

def _spread_keys(kernels, count, cap, S, seed):
    """Distinct keys none of whose chains leaves its slice."""
    g = torch.Generator().manual_seed(seed)
    keys = torch.unique(torch.randint(0, 2**40, (2 * count,),
                                      dtype=torch.int64, generator=g))
    # no home in the last 64 slots of a slice, no run of 64 taken slots
    keys = keys[_home_slots(kernels, keys, cap) % S < S - 64][:count]
    worst, left = _probe(_home_slots(kernels, keys, cap), cap, S)
    assert sum(left) == 0 and worst < 64, (worst, left)
    return keys


@gpu
@both
def test_heavy_key_among_uniform_rows(kernels, monkeypatch, T, owned):
    cap, B = 4096, 8
    uni = _spread_keys(kernels, 600, cap, cap // B, 41)
    heavy = uni[0]
    g = torch.Generator().manual_seed(42)
    keys = torch.cat([heavy.repeat(5 * T),
                      uni[torch.randint(0, uni.shape[0], (T,),
                                        generator=g)]])
    keys = keys[torch.randperm(keys.shape[0], generator=g)]
    batches = [(keys, _vals(keys.shape[0], 43))]
    _check(kernels, monkeypatch, owned, batches, 1)
    if owned == "1":
        clean, totals, _, _, table = _direct(kernels, keys, batches[0][1],
                                             cap, B)
        hb = int(_home_slots(kernels, heavy.reshape(1), cap)) // (cap // B)
        LIMIT = kernels.PART_OWN_LIMIT
        assert int(totals[hb]) >= 5 * T > LIMIT
        want = torch.zeros(B, dtype=torch.int64)
        want[hb] = totals[hb] - LIMIT  # no chain leaves a slice: 0 spills
        assert torch.equal(clean, want)
        k, s = _table_result(kernels, table)
        want_k, want_s = _cpu_oracle(batches)
        assert torch.equal(k, want_k) and torch.equal(s, want_s)


@gpu
@both
@pytest.mark.parametrize("which", ["LIMIT", "LIMIT+1", "3T+17"])
def test_all_rows_on_one_key(kernels, monkeypatch, T, owned, which):
    LIMIT = kernels.PART_OWN_LIMIT
    n = {"LIMIT": LIMIT, "LIMIT+1": LIMIT + 1, "3T+17": 3 * T + 17}[which]
    keys = torch.full((n,), 424242, dtype=torch.int64)
    batches = [(keys, _vals(n, 44))]
    _check(kernels, monkeypatch, owned, batches, 1)
    if owned == "1":
        cap, B = 4096, 4
        clean, totals, _, _, table = _direct(kernels, keys, batches[0][1],
                                             cap, B)
        hb = int(_home_slots(kernels, keys[:1], cap)) // (cap // B)
        want = torch.zeros(B, dtype=torch.int64)
        want[hb] = n - LIMIT
        assert int(totals[hb]) == n and torch.equal(clean, want)
        k, s = _table_result(kernels, table)
        want_k, want_s = _cpu_oracle(batches)
        assert torch.equal(k, want_k) and torch.equal(s, want_s)


# ------------------------------------------------------- key write-back skip

@gpu
@both
def test_new_keys_same_keys_new_keys(kernels, monkeypatch, T, owned):
    g = torch.Generator().manual_seed(51)
    a = torch.randperm(3000, generator=g) * 7919 - 1000
    b = torch.randperm(3000, generator=g) * 104729 + 5
    n = 2 * T + 3
    batches = []
    for i, src in enumerate([a, a, torch.cat([a[:500], b])]):
        idx = torch.cat([torch.arange(src.shape[0]),
                         torch.randint(0, src.shape[0],
                                       (n - src.shape[0],), generator=g)])
        batches.append((src[idx], _vals(n, 52 + i)))
    _check(kernels, monkeypatch, owned, batches, 3)


# ------------------------------------------------------------- sentinel rows

@gpu
@both
def test_sentinel_rows(kernels, monkeypatch, T, owned):
    n = 3 * T + 17
    g = torch.Generator().manual_seed(4)
    keys = torch.randint(0, 1000, (n,), dtype=torch.int64, generator=g)
    keys[::11] = kernels.GB_SENTINEL
    vals = _vals(n, 4)
    table = _check(kernels, monkeypatch, owned, [(keys, vals)], 1)
    assert int(table.flags[0].item()) == 1  # sentinel_seen
    want = vals[::11].sum()  # wraps like the table's adds
    assert int(table.tabs[0][table.cap].item()) == int(want)


@gpu
@both
def test_no_sentinel_flag_without_sentinel_rows(kernels, monkeypatch, T,
                                                owned):
    n = T + 1
    keys = torch.arange(n, dtype=torch.int64) % 300
    table = _check(kernels, monkeypatch, owned, [(keys, _vals(n, 5))], 1)
    assert int(table.flags[0].item()) == 0


# -------------------------------------------------------------------- regrow

@gpu
@both
def test_regrow(kernels, monkeypatch, owned):
    # 100k distinct keys into a 1024-slot table: overflow flag, regrow,
    # re-insert of the retained (unpartitioned) batches
    g = torch.Generator().manual_seed(7)
    keys = torch.cat([torch.randperm(100_000, generator=g),
                      torch.randperm(100_000, generator=g)]) * 31 - 5
    batches = [(keys, _vals(keys.shape[0], 7))]
    want_k, want_s = _cpu_oracle(batches)
    pk, ps, table, calls = _run(kernels, monkeypatch, "part", owned, batches,
                                cap_hint=1024)
    assert len(calls) >= 2, calls  # first insert + re-insert after regrow
    assert all(c == int(owned) for c in calls), calls
    assert table.cap > 1024
    assert torch.equal(pk, want_k) and torch.equal(ps, want_s)


# --------------------------------------------------------------- fan-out rule

def test_owned_fanout_rule():
    from bigslice_amd.kernels import part_owned_buckets as f
    slots, tile, maxb = 4096, 8192, 1024
    # flagship: 125M rows in 16 batches, 1M keys -> cap 4M
    assert f(125_000_000 // 16, 1 << 22, slots, tile, maxb) == (1024, 4096)
    # 64k keys -> cap 256k: the row count sets the fan-out
    assert f(125_000_000 // 16, 1 << 18, slots, tile, maxb) == (1024, 256)
    # cap 8M would need slices of 8192 slots
    assert f(125_000_000 // 16, 1 << 23, slots, tile, maxb) is None
    # a tiny table clamps the fan-out to its capacity
    assert f(125_000_000 // 16, 256, slots, tile, maxb) == (256, 1)
    # few rows: the lower clamp
    assert f(1, 1024, slots, tile, maxb) == (2, 512)
    assert f(3 * tile + 17, 1024, slots, tile, maxb) == (4, 256)
    # the capacity term alone
    assert f(tile, 1 << 20, slots, tile, maxb) == (256, 4096)
