"""Kernel micro-benchmarks (for rocprofv3/PMC runs and A/B timing).

  python -m bigslice_amd.tools.microprof groupby --rows 125000000
  python -m bigslice_amd.tools.microprof partition --rows 125000000
  python -m bigslice_amd.tools.microprof hash --rows 125000000
  python -m bigslice_amd.tools.microprof tokenize --iters 20
  python -m bigslice_amd.tools.microprof groupby_multi --rows 8388608
  python -m bigslice_amd.tools.microprof runs_multi --rows 8388608
  python -m bigslice_amd.tools.microprof iddict --rows 8388608
  python -m bigslice_amd.tools.microprof bytes_gather
  python -m bigslice_amd.tools.microprof sample --nkeys 1000000
  python -m bigslice_amd.tools.microprof finish --nkeys 1000000 --nparts 8

Times each kernel phase with hipEvents over --iters iterations.  Keep
runs short: this is the target for `rocprofv3 --pmc ... -- ...`.
"""

from __future__ import annotations

import argparse
import json
import os

import torch

from bigslice_amd import kernels
from bigslice_amd.frame import Frame


def timeit(fn, iters):
    """Median of per-iteration times (2 warmups).  Median, not mean:
    on leases where a prior process ran, the FIRST touch of each
    freshly-committed GPU allocation pays a one-time ~40-80 ms
    driver-side cost (measured: iteration k hits it when the caching
    allocator grows, all later iterations are clean) — a mean smears
    that one-time cost into a phantom 3-4x 'regression'."""
    import time
    for _ in range(2):
        fn()  # warmups absorb allocator-growth first-touch costs
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(iters, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1000)
    ts.sort()
    return ts[len(ts) // 2]


def tokenize_ab(dev, g, iters, nbytes=64 << 20):
    """BytesColumn.split on one warm batch of synthetic text (8-byte
    words, single spaces, 64-byte lines, one row per line): the K20
    kernels against split_torch on the same device tensors, in this
    process.  Wall time per call, readback of the totals included."""
    from bigslice_amd.frame import BytesColumn, split_torch
    nlines = nbytes // 64
    text = torch.randint(97, 123, (nlines, 64), dtype=torch.uint8,
                         device=dev, generator=g)
    text[:, 8::9] = 32
    text[:, 63] = 10
    col = BytesColumn(
        text.flatten(),
        torch.arange(nlines + 1, dtype=torch.int64, device=dev) * 64)
    mask4 = kernels.tokenize_mask(None)
    out = {"which": "tokenize", "bytes": nbytes, "rows": nlines}
    for with_rows in (False, True):
        nat = kernels.tokenize_bytes(col.data, col.offsets, mask4,
                                     with_rows)
        ref = split_torch(col.data, col.offsets, mask4, with_rows)
        assert all(torch.equal(a, b) for a, b in zip(nat, ref))
        out["tokens"] = nat[1].shape[0] - 1
        del nat, ref
        tag = "_rows" if with_rows else ""
        # the torch path first: it has the larger footprint, so the
        # allocator is at its peak before either arm is timed
        t_ms = timeit(lambda: split_torch(col.data, col.offsets, mask4,
                                          with_rows), iters)
        n_ms = timeit(lambda: kernels.tokenize_bytes(
            col.data, col.offsets, mask4, with_rows), iters)
        out["torch%s_ms" % tag] = t_ms
        out["native%s_ms" % tag] = n_ms
        out["torch%s_gbps" % tag] = nbytes / t_ms / 1e6
        out["native%s_gbps" % tag] = nbytes / n_ms / 1e6
    out["split_ms"] = timeit(lambda: col.split(), iters)
    return out


def groupby_multi(dev, g, iters, rows, nkeys, ncols, cap):
    """The two launches of the multi-column insert (K21), each on its
    own, over one batch into a presized warm table (every tuple present
    after the warmups: pure probe / compare + atomicAdd), then the whole
    insert and the table's compaction."""
    from bigslice_amd.kernels import groupby_multi as gbm
    C = kernels._C
    # tuples: mixed-radix digits of a number below nkeys
    ids = torch.randint(0, nkeys, (rows,), dtype=torch.int64, device=dev,
                        generator=g)
    radix = int(round(nkeys ** (1.0 / ncols))) + 1
    keys = [((ids // radix ** c) % radix).contiguous()
            for c in range(ncols)]
    del ids
    vals = [torch.ones(rows, dtype=torch.int64, device=dev)]
    t = gbm.MultiKeyTable(ncols, [torch.int64], ["sum"], dev)
    t._alloc(cap or kernels._next_pow2(4 * nkeys))
    fp = t.opts.fp_bits
    out = {"which": "groupby_multi", "rows": rows, "nkeys": nkeys,
           "key_cols": ncols, "cap": t.cap}
    slots = C.groupby_mk_claim(keys, t.tags, t.kcols, t.flags,
                               kernels.MAX_PROBES, fp)
    out["claim_ms"] = timeit(
        lambda: C.groupby_mk_claim(keys, t.tags, t.kcols, t.flags,
                                   kernels.MAX_PROBES, fp), iters)
    out["accum_ms"] = timeit(
        lambda: C.groupby_mk_accum(keys, vals, t.codes, slots, t.tags,
                                   t.kcols, t.tabs, t.flags), iters)
    out["insert_ms"] = timeit(
        lambda: C.groupby_mk_insert(keys, vals, t.codes, t.tags, t.kcols,
                                    t.tabs, t.flags, kernels.MAX_PROBES,
                                    fp), iters)

    def compact():
        cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        C.groupby_compact(t.tags, t.kcols + t.tabs, cursor)
    out["compact_ms"] = timeit(compact, iters)
    flags = t.flags.tolist()
    assert flags[1] == 0 and flags[2] == 0, flags
    out["distinct"] = int((t.tags[:t.cap] != kernels.GB_SENTINEL).sum())
    # streamed bytes per row: K key columns read by both launches, the
    # slot written and read, the value column read
    stream = rows * (2 * 8 * ncols + 2 * 4 + 8)
    out["insert_stream_gbps"] = stream / out["insert_ms"] / 1e6
    out["accum_gatomics_per_s"] = rows / out["accum_ms"] / 1e6
    out["grows_per_sec"] = rows / out["insert_ms"] / 1e6
    return out


def runs_multi(dev, g, iters, rows, nkeys, ncols):
    """The K22 primitives on one warm batch: run boundaries of `rows`
    lexicographically sorted tuples over about `nkeys` distinct ones
    (count + scan + write, no readback), beside k_runs_sorted on one
    column of the same length, and the lexicographic search of nkeys
    query tuples into the distinct tuples, beside torch.searchsorted on
    scalars of the same sizes."""
    C = kernels._C
    ids = torch.sort(torch.randint(0, nkeys, (rows,), dtype=torch.int64,
                                   device=dev, generator=g)).values
    radix = int(round(nkeys ** (1.0 / ncols))) + 1
    # mixed-radix digits, most significant first: sorted as tuples
    cols = [((ids // radix ** (ncols - 1 - c)) % radix).contiguous()
            for c in range(ncols)]
    out = {"which": "runs_multi", "rows": rows, "nkeys": nkeys,
           "key_cols": ncols}
    uniq, starts, cnt = C.runs_multi(cols)
    u = int(cnt.item())
    ref = torch.unique_consecutive(ids)
    assert u == ref.shape[0], (u, ref.shape[0])
    out["distinct"] = u
    out["runs_multi_ms"] = timeit(lambda: C.runs_multi(cols), iters)
    out["runs_sorted_1col_ms"] = timeit(lambda: C.runs_sorted(ids), iters)
    # the keys are read twice: 2 x NK x 8 B per row
    out["runs_multi_gbps"] = (rows * 2 * ncols * 8
                              / out["runs_multi_ms"] / 1e6)
    out["runs_sorted_1col_gbps"] = rows * 8 / out["runs_sorted_1col_ms"] / 1e6
    table = [x[:u].contiguous() for x in uniq]
    pick = torch.randint(0, u, (nkeys,), dtype=torch.int64, device=dev,
                         generator=g)
    query = [t[pick].contiguous() for t in table]
    query[-1] = query[-1] + torch.randint(0, 2, (nkeys,), dtype=torch.int64,
                                          device=dev, generator=g)
    out["queries"] = nkeys
    out["lex_search_ms"] = timeit(
        lambda: C.lex_searchsorted(table, query, False), iters)
    q1 = ref[pick].contiguous()
    out["torch_searchsorted_1col_ms"] = timeit(
        lambda: torch.searchsorted(ref, q1), iters)
    return out


def _hex_words(idx):
    """Row i is the 8 hex digits of idx[i], lowest first: distinct
    numbers give distinct 8-byte strings."""
    from bigslice_amd.frame import BytesColumn
    digits = torch.tensor(list(b"0123456789abcdef"), dtype=torch.uint8,
                          device=idx.device)
    shifts = torch.arange(0, 32, 4, device=idx.device)
    data = digits[(idx[:, None] >> shifts) & 15].flatten()
    offsets = torch.arange(idx.shape[0] + 1, dtype=torch.int64,
                           device=idx.device) * 8
    return BytesColumn(data, offsets)


def iddict(dev, g, iters, rows, nkeys, cap):
    """The id dictionary (K23) over one batch of `rows` 8-byte strings
    from `nkeys` distinct ones, into a presized table.  Warm (every id
    present after the warmups: pure probe, as claim_ms of groupby_multi):
    the claim, the lookup and a whole add with its one readback.  Fresh:
    a whole add into an empty presized dictionary, the gather of the
    exemplars included."""
    C = kernels._C
    col = _hex_words(torch.randint(0, nkeys, (rows,), dtype=torch.int64,
                                   device=dev, generator=g))
    ids = col.ids64()
    lens = col.lengths().contiguous()
    cap = cap or kernels._next_pow2(4 * nkeys)
    d = kernels.IdDictionary(dev, cap_hint=cap)
    d.add(ids, col)
    assert d.regrows == 0 and d.cap == cap, (d.regrows, d.cap)
    out = {"which": "iddict", "rows": rows, "nkeys": nkeys, "cap": d.cap,
           "distinct": len(d)}
    pos = d.lookup(ids)
    assert int(pos.min()) >= 0
    k = min(rows, 1 << 20)
    back = d.strings().gather(pos[:k])
    assert torch.equal(back.data, col.data[:8 * k])
    del pos, back
    counters = torch.zeros(3, dtype=torch.int64, device=dev)
    out["claim_ms"] = timeit(
        lambda: C.iddict_claim(ids, lens, d.tags, d.ref, len(d), counters,
                               kernels.MAX_PROBES), iters)
    assert counters.tolist() == [0, 0, 0], counters.tolist()
    out["lookup_ms"] = timeit(
        lambda: C.iddict_lookup(ids, d.tags, d.ref, kernels.MAX_PROBES),
        iters)
    out["add_warm_ms"] = timeit(lambda: d.add(ids, col), iters)
    # a readback on an idle stream: what the add's one readback costs
    # beyond waiting for the claim
    out["readback_ms"] = timeit(
        lambda: torch.zeros(3, dtype=torch.int64, device=dev).tolist(),
        iters)
    out["readback_share_of_add"] = out["readback_ms"] / out["add_warm_ms"]

    def fresh():
        f = kernels.IdDictionary(dev, cap_hint=cap)
        f.add(ids, col)
    out["add_fresh_ms"] = timeit(fresh, iters)
    out["claim_grows_per_s"] = rows / out["claim_ms"] / 1e6
    out["lookup_grows_per_s"] = rows / out["lookup_ms"] / 1e6
    return out


def bytes_gather_ab(dev, g, iters, rows=1 << 20):
    """BytesColumn.gather (K23, csrc/bytes_gather.hip) against
    BytesColumn.select on the same random indices: `rows` rows of 4..12
    bytes and `rows` rows of 64 bytes, one readback each included."""
    from bigslice_amd.frame import BytesColumn
    out = {"which": "bytes_gather", "rows": rows}
    for tag, lo, hi in (("short", 4, 12), ("long", 64, 64)):
        lens = torch.randint(lo, hi + 1, (rows,), dtype=torch.int64,
                             device=dev, generator=g)
        offsets = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        total = int(offsets[-1])
        col = BytesColumn(torch.randint(0, 256, (total,), dtype=torch.uint8,
                                        device=dev, generator=g), offsets)
        idx = torch.randint(0, rows, (rows,), dtype=torch.int64, device=dev,
                            generator=g)
        want, got = col.select(idx), col.gather(idx)
        assert torch.equal(want.data, got.data)
        assert torch.equal(want.offsets, got.offsets)
        nbytes = int(want.data.shape[0])
        del want, got
        s_ms = timeit(lambda: col.select(idx), iters)
        g_ms = timeit(lambda: col.gather(idx), iters)
        k_ms = timeit(lambda: col.gather(idx, total=nbytes), iters)
        out[tag] = {"bytes": nbytes, "select_ms": s_ms, "gather_ms": g_ms,
                    "gather_known_total_ms": k_ms,
                    "select_gbps": nbytes / s_ms / 1e6,
                    "gather_gbps": nbytes / g_ms / 1e6,
                    "gather_known_total_gbps": nbytes / k_ms / 1e6}
    return out


def sample_ab(dev, g, iters, rows, nkeys):
    """The cardinality sample of GroupTable over one prefix of `rows`
    keys from `nkeys`: the sorted prefix with its key-change count (24
    launches at 2^19 rows) against the one counting kernel (2 launches).
    Wall time per call, the readback of the count included, as
    _read_sample pays it."""
    C = kernels._C
    keys = torch.randint(0, nkeys, (rows,), dtype=torch.int64, device=dev,
                         generator=g)

    def by_sort():
        sk = C.radix_sort_keys(keys, probe=False)
        return int((sk[1:] != sk[:-1]).sum().item())

    def by_hash():
        return int(C.groupby_sample_distinct(keys, rows).item())
    assert by_sort() == by_hash()
    return {"which": "sample", "rows": rows, "nkeys": nkeys,
            "distinct": by_hash() + 1,
            "sort_ms": timeit(by_sort, iters),
            "hash_ms": timeit(by_hash, iters)}


def finish_ab(dev, g, iters, nkeys, cap, nparts):
    """Finish of one filled table of `cap` slots and `nkeys` keys into
    `nparts` partitions: compaction, its readback, hash_partition and its
    readback (GroupTable.finish + split_frame) against the fused
    groupby_compact_partition and its one readback."""
    C = kernels._C
    cap = cap or kernels._next_pow2(4 * nkeys)
    t = kernels.GroupTable([torch.int64], ["sum"], dev)
    t._alloc(cap)
    keys = torch.randperm(nkeys, dtype=torch.int64, device=dev, generator=g)
    C.groupby_insert(keys, [torch.ones_like(keys)], t.codes, t.tkeys,
                     t.tabs, t.flags, kernels.MAX_PROBES)
    assert t.flags.tolist() == [0, 0]

    def old():
        outs, (n, _, _) = t._compact()
        cols = [o[:n] for o in outs]
        return C.hash_partition(cols, [cols[0]], nparts, 0)[1].tolist()

    def fused():
        host = C.groupby_compact_partition(t.tkeys, t.tabs, t.flags,
                                           nparts)[1]
        return host.tolist()[:nparts]
    assert old() == fused()
    return {"which": "finish", "nkeys": nkeys, "cap": cap, "nparts": nparts,
            "old_ms": timeit(old, iters), "fused_ms": timeit(fused, iters)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", choices=["groupby", "groupby_part", "insert",
                                      "sample", "finish",
                                      "groupby_multi", "runs_multi",
                                      "partition", "hash", "compact",
                                      "sortcombine", "sortcombine2", "hashbytes",
                                      "runs", "tokenize", "iddict",
                                      "bytes_gather"])
    ap.add_argument("--cap", type=int, default=0,
                    help="table capacity (0 = 2x nkeys rounded up)")
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--nkeys", type=int, default=1_000_000)
    ap.add_argument("--nparts", type=int, default=8)
    ap.add_argument("--key-cols", type=int, default=2,
                    help="key columns of groupby_multi and runs_multi")
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available() and kernels.have_extension()
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    if args.which == "tokenize":
        print(json.dumps(tokenize_ab(dev, g, args.iters)))
        return
    if args.which == "iddict":
        print(json.dumps(iddict(dev, g, args.iters, args.rows, args.nkeys,
                                args.cap)))
        return
    if args.which == "bytes_gather":
        print(json.dumps(bytes_gather_ab(dev, g, args.iters)))
        return
    if args.which == "sample":
        print(json.dumps(sample_ab(dev, g, args.iters,
                                   min(args.rows, 1 << 19), args.nkeys)))
        return
    if args.which == "finish":
        print(json.dumps(finish_ab(dev, g, args.iters, args.nkeys, args.cap,
                                   args.nparts)))
        return
    if args.which == "groupby_multi":
        print(json.dumps(groupby_multi(dev, g, args.iters, args.rows,
                                       args.nkeys, args.key_cols,
                                       args.cap)))
        return
    if args.which == "runs_multi":
        print(json.dumps(runs_multi(dev, g, args.iters, args.rows,
                                    args.nkeys, args.key_cols)))
        return
    keys = torch.randint(0, args.nkeys, (args.rows,), dtype=torch.int64,
                         device=dev, generator=g)
    vals = torch.ones(args.rows, dtype=torch.int64, device=dev)

    out = {"which": args.which, "rows": args.rows, "nkeys": args.nkeys}
    if args.which == "groupby":
        def run():
            t = kernels.GroupTable([torch.int64], ["sum"], dev)
            t.insert(keys, [vals])
            t.finish()
        ms = timeit(run, args.iters)
    elif args.which == "groupby_part":
        # partitioned LDS pre-aggregation (K19): per-batch kernel times
        # of histogram+offsets+scatter, of the aggregate pass, and of
        # the plain one-pass insert over the same batch and warm table
        n = min(args.rows, int(os.environ.get("PART_BATCH", 8 << 20)))
        bk, bv = keys[:n].contiguous(), vals[:n].contiguous()
        cap = args.cap or kernels._next_pow2(4 * args.nkeys)
        B = int(os.environ.get("PART_BUCKETS", "0")) or \
            kernels.part_buckets(n, args.nkeys, cap)
        t = kernels.GroupTable([torch.int64], ["sum"], dev)
        t._alloc(cap)
        C = kernels._C
        # scatter tiles per workgroup: PART_GROUP forces it, 0 = the rule
        G = int(os.environ.get("PART_GROUP", "0"))
        pairs, _ = C.groupby_part_scatter(bk, bv, cap, B, G)
        out.update(rows=n, cap=cap, buckets=B,
                   group_tiles=G or C.groupby_part_group_tiles(n))
        out["scatter_ms"] = timeit(
            lambda: C.groupby_part_scatter(bk, bv, cap, B, G), args.iters)
        out["aggregate_ms"] = timeit(
            lambda: C.groupby_part_aggregate(
                pairs, t.tkeys, t.tabs[0], t.flags, kernels.MAX_PROBES),
            args.iters)
        out["part_ms"] = timeit(
            lambda: C.groupby_insert_part(
                bk, bv, t.tkeys, t.tabs[0], t.flags, kernels.MAX_PROBES,
                B, 0, G), args.iters)
        out["plain_ms"] = timeit(
            lambda: C.groupby_insert(
                bk, [bv], t.codes, t.tkeys, t.tabs, t.flags,
                kernels.MAX_PROBES), args.iters)
        # bucket-owning aggregate (owner + cleanup passes) at its own
        # fan-out, against the tiled aggregate above
        own = kernels.part_owned_buckets(
            n, cap, kernels.PART_LDS_SLOTS, kernels.PART_TILE_ROWS,
            kernels.PART_MAX_BUCKETS)
        if own is not None:
            Bo = own[0]
            out["owned_buckets"], out["owned_slice"] = own
            out["owned_scatter_ms"] = timeit(
                lambda: C.groupby_part_scatter(bk, bv, cap, Bo, G),
                args.iters)
            po, to = C.groupby_part_scatter(bk, bv, cap, Bo, G)
            # rows the owners leave to the cleanup pass: an upper bound
            # on the global atomics that remain.  Taken on the first run
            # (spilled rows overwrite consumed ones, so the buffer is
            # good for timing afterwards, not for results)
            clean = C.groupby_part_owned(po, to, t.tkeys, t.tabs[0],
                                         t.flags, kernels.MAX_PROBES)
            out["cleanup_rows"] = int(clean.sum())
            out["owned_aggregate_ms"] = timeit(
                lambda: C.groupby_part_owned(
                    po, to, t.tkeys, t.tabs[0], t.flags,
                    kernels.MAX_PROBES), args.iters)
            out["owned_part_ms"] = timeit(
                lambda: C.groupby_insert_part(
                    bk, bv, t.tkeys, t.tabs[0], t.flags,
                    kernels.MAX_PROBES, Bo, 1, G), args.iters)
        assert int(t.flags[1].item()) == 0, "table overflow"
        # global atomics of one aggregate pass = rows that missed the
        # LDS tables + flushed slots; counted on a fresh table as the
        # sum of a ones column
        t2 = kernels.GroupTable([torch.int64], ["sum"], dev)
        t2._alloc(cap)
        ones = torch.ones_like(pairs)
        ones[:, 0] = pairs[:, 0]
        C.groupby_part_aggregate(ones, t2.tkeys, t2.tabs[0], t2.flags,
                                 kernels.MAX_PROBES)
        out["distinct_in_batch"] = int((t2.tkeys[:cap]
                                        != kernels.GB_SENTINEL).sum())
        # distinct keys per aggregate tile, summed: the flushed slots (a
        # lower bound on the pass's global atomics; LDS-table misses add
        # one each)
        T = kernels.PART_TILE_ROWS
        full = (n // T) * T
        tk = pairs[:full, 0].reshape(-1, T).sort(dim=1).values
        flushed = int((tk[:, 1:] != tk[:, :-1]).sum()) + tk.shape[0]
        if full < n:
            flushed += int(pairs[full:, 0].unique().shape[0])
        out["flushed_slots"] = flushed
        args.rows = n
        ms = out["part_ms"]
    elif args.which in ("insert", "compact"):
        # insert: steady-state rate of the plain one-pass insert into a
        # presized table (all keys present after warmup: pure
        # probe+atomicAdd); compact: compaction of that filled table
        cap = args.cap or kernels._next_pow2(2 * args.nkeys)
        t = kernels.GroupTable([torch.int64], ["sum"], dev)
        t._alloc(cap)
        out["cap"] = cap

        def insert():
            kernels._C.groupby_insert(keys, [vals], t.codes, t.tkeys,
                                      t.tabs, t.flags, 4096)

        def compact():
            cursor = torch.zeros(1, dtype=torch.int64, device=dev)
            kernels._C.groupby_compact(t.tkeys, t.tabs, cursor)
        if args.which == "compact":
            insert()
        ms = timeit(insert if args.which == "insert" else compact,
                    args.iters)
        assert int(t.flags[1].item()) == 0, "table overflow"
    elif args.which == "runs":
        # K18 run-boundary compaction over sorted keys (PMC target)
        sk = torch.sort(keys).values.contiguous()

        def run():
            kernels._C.runs_sorted(sk)
        ms = timeit(run, args.iters)
    elif args.which == "partition":
        f = Frame([keys, vals], prefix=1)

        def run():
            kernels.partition_frame(f, args.nparts, None)
        ms = timeit(run, args.iters)
    elif args.which == "hash":
        def run():
            kernels.hash_columns_device([keys], 0)
        ms = timeit(run, args.iters)
    else:
        ms = None
    if ms is not None:
        out["ms"] = ms
        out["grows_per_sec"] = args.rows / ms / 1e6
    if args.which in ("sortcombine", "sortcombine2"):
        # production sort_combine, one arm forced: sortcombine = rocPRIM
        # reduce-by-key, sortcombine2 = K18 boundaries + thread-per-run
        from bigslice_amd.kernels.sortedkeys import sort_combine
        arm = "rocprim" if args.which == "sortcombine" else "runs"
        out["ms"] = timeit(
            lambda: sort_combine(keys, [vals], [0], arm=arm), args.iters)
        out["grows_per_s"] = args.rows / out["ms"] / 1e6
    if args.which == "hashbytes":
        import random

        from bigslice_amd import strings
        rng = random.Random(2)
        words = ["w%05d" % rng.randrange(args.nkeys)
                 for _ in range(min(args.rows, 10_000_000))]
        data, offs = strings.pack_strings(words)
        b, o = strings.to_device(data, offs, "cuda:0")
        from bigslice_amd.kernels import _C

        def run():
            _C.hash_bytes64(b, o, 0x9ACB0442, 0x85EBCA6B)
        out["ms"] = timeit(run, args.iters)
        out["rows"] = len(words)
        out["mwords_per_s"] = len(words) / out["ms"] / 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
