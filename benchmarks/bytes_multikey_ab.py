"""A/B: Reduce over the composite key (word: bytes, doc: int), the host
path (DictAggregator: one .cpu().tolist() per column and a Python dict
of tuples, what every GPU session ran for such keys before K23 and
still runs under BIGSLICE_GB_BYTES_MULTIKEY=0) against the device path
(BytesTupleAggregator: id dictionary + MultiKeyTable).

One process, one session, the same device tensors for both arms, runs
interleaved.  Input: --rows rows of (word, doc, 1) over a --vocab-word
vocabulary and --docs documents, in --shards shards.  A step is
`sess.run(...)` plus `discard()`.  Both arms must give equal results,
as sets of rows, before anything is timed.  The host arm stops after
three runs when one of them takes more than 10 s.

After the A/B, the device arm's step is taken apart on one shard's
frame: ids, claim (the dictionary's add without the gather), gather,
table insert, finish.

    python benchmarks/bytes_multikey_ab.py [--runs 5] [--rows 4194304]

Prints one JSON line and a summary.  The bar: the device arm's slowest
run below the host arm's fastest.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import bigslice_amd as bs  # noqa: E402
from bigslice_amd import kernels  # noqa: E402
from bigslice_amd.frame import BytesColumn  # noqa: E402

DEV = "cuda:0"
SWITCH = "BIGSLICE_GB_BYTES_MULTIKEY"
_DATA = {}


def build(nshard):
    def gen(shard, ctx):
        yield _DATA[shard]
    src = bs.ReaderFunc(nshard, gen, bs.schema_of(bytes, int, int))
    return bs.Reduce(bs.Prefixed(src, 2), "sum")


FV = bs.func(build)


def sync():
    torch.cuda.synchronize()


def once(sess, nshard, switch):
    os.environ[SWITCH] = switch
    sync()
    t0 = time.perf_counter()
    res = sess.run(FV, nshard)
    res.discard()
    sync()
    return (time.perf_counter() - t0) * 1000


def result(sess, nshard, switch):
    os.environ[SWITCH] = switch
    res = sess.run(FV, nshard)
    rows = list(res.scan())
    res.discard()
    as_set = set(rows)
    assert len(as_set) == len(rows), "a key came out twice"
    return as_set


def timed(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return out, (time.perf_counter() - t0) * 1000


def phases(dev, nshard, runs):
    """Where the device arm's producer step goes, on shard 0's frame:
    medians over `runs` repetitions, each into fresh tables."""
    from bigslice_amd.kernels.groupby_multi import MultiKeyTable
    from bigslice_amd.ops.aggregate import Aggregation, _combine_once
    C = kernels._C
    agg = Aggregation(["sum"])
    words, docs, ones = _DATA[0]
    n = len(words)
    acc = {k: [] for k in ("ids", "claim", "gather", "insert", "finish",
                           "lookup_gather_out")}
    for _ in range(runs + 1):  # the first repetition warms the allocator
        ids, t = timed(words.ids64)
        acc["ids"].append(t)
        d = kernels.IdDictionary(dev)
        d.cap = kernels._next_pow2(2 * n)  # what add() takes for n rows
        d.tags, d.ref = d._alloc(d.cap)
        lens = words.lengths().contiguous()
        counters = torch.zeros(3, dtype=torch.int64, device=dev)

        def claim():
            rows = C.iddict_claim(ids, lens, d.tags, d.ref, len(d),
                                  counters, kernels.MAX_PROBES)
            return rows, counters.tolist()
        (newrows, (m, nbytes, overflow)), t = timed(claim)
        assert not overflow
        acc["claim"].append(t)
        ex, t = timed(lambda: words.gather(newrows[:m], total=nbytes))
        acc["gather"].append(t)
        table = MultiKeyTable(2, [torch.int64], ["sum"], dev,
                              fallback=lambda k, v: _combine_once(k, v, agg))
        _, t = timed(lambda: table.insert([ids, docs], [ones]))
        acc["insert"].append(t)
        (gk, _), t = timed(table.finish)
        acc["finish"].append(t)
        d2 = kernels.IdDictionary(dev)
        d2.add(ids, words)
        _, t = timed(lambda: d2.strings().gather(d2.lookup(gk[0])))
        acc["lookup_gather_out"].append(t)
    return {"rows": n, **{k + "_ms": round(statistics.median(v[1:]), 3)
                          for k, v in acc.items()}}


def mmm(ts):
    return [round(min(ts), 3), round(statistics.median(ts), 3),
            round(max(ts), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--vocab", type=int, default=20_000)
    ap.add_argument("--docs", type=int, default=64)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--device", default=DEV)
    args = ap.parse_args()
    assert args.runs >= 5, "at least five interleaved runs per arm"
    dev, nshard = args.device, args.shards
    g = torch.Generator(device=dev)
    g.manual_seed(23)
    per = args.rows // nshard
    vocab = BytesColumn.from_list(
        [b"w%x" % (i * 2654435761 % (1 << 32)) for i in range(args.vocab)],
        dev)
    for s in range(nshard):
        w = torch.randint(0, args.vocab, (per,), dtype=torch.int64,
                          device=dev, generator=g)
        docs = torch.randint(0, args.docs, (per,), dtype=torch.int64,
                             device=dev, generator=g)
        _DATA[s] = (vocab.select(w), docs,
                    torch.ones(per, dtype=torch.int64, device=dev))
    sess = bs.start(parallelism=nshard, device=dev)
    want = result(sess, nshard, "0")
    got = result(sess, nshard, "1")
    assert want == got, "arms differ"
    groups = len(want)
    del want, got
    print("arms agree on %d rows" % groups, file=sys.stderr, flush=True)
    once(sess, nshard, "1")  # warm the allocator
    th, td = [], []
    for i in range(args.runs):
        host = "skipped"
        if not (i >= 3 and max(th) > 10_000):
            th.append(once(sess, nshard, "0"))
            host = "%.1f ms" % th[-1]
        td.append(once(sess, nshard, "1"))
        print("run %d: host %s, device %.2f ms" % (i, host, td[-1]),
              file=sys.stderr, flush=True)
    os.environ.pop(SWITCH, None)
    sess.shutdown()
    rec = {
        "rows": per * nshard, "groups": groups, "vocab": args.vocab,
        "docs": args.docs, "shards": nshard, "runs": args.runs,
        "device": dev,
        "host_ms": [round(x, 3) for x in th],
        "device_ms": [round(x, 3) for x in td],
        "host_min_med_max": mmm(th), "device_min_med_max": mmm(td),
        "device_slowest_below_host_fastest": max(td) < min(th),
        "host_over_device_median": round(
            statistics.median(th) / statistics.median(td), 1),
        "device_phases_one_shard": phases(dev, nshard, args.runs),
    }
    print(json.dumps(rec), flush=True)
    print("%d rows, %d groups, %d shards, ms min/med/max" % (
        per * nshard, groups, nshard))
    for name, key in (("host path (switch off)", "host_min_med_max"),
                      ("device path", "device_min_med_max")):
        print("  %-24s %s" % (name, " / ".join("%.2f" % x for x in rec[key])))
    print("  device slowest below host fastest:",
          rec["device_slowest_below_host_fastest"])
    print("  device phases, one shard of %d rows (ms):" % per)
    for k, v in rec["device_phases_one_shard"].items():
        if k != "rows":
            print("    %-22s %.3f" % (k[:-3], v))


if __name__ == "__main__":
    main()
