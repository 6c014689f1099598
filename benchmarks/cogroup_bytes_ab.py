"""A/B: Cogroup of two slices keyed by strings, the host path (a Python
dict of bytes or of tuples, what every GPU session ran for such keys
before K24 and still runs under BIGSLICE_COGROUP_BYTES=0) against the
device path (grouping by 64-bit ids through the K22 steps, then the
byte-order ranks of the union's distinct strings).

One process, one session, the same device columns for both arms, runs
interleaved.  Inputs: two slices of --rows rows each, one int64 value
column per side, over a vocabulary of --vocab words b"term-<i>":
  word       key (word), words drawn from the whole vocabulary
  word_doc   key (word, doc), vocab/16 words x 16 docs
  int64      the single-int64-key device cogroup of the same row and key
             counts, to state what the strings cost
A step is `sess.run(...)` plus `discard()`.  Both arms must give equal
results before anything is timed: per output frame the same keys in the
same order, and per key and side the same multiset of values.

    python benchmarks/cogroup_bytes_ab.py [--runs 5] [--rows 4194304]

Prints one JSON line and a summary.  The bar: the device arm's slowest
run below the host arm's fastest, for both key shapes.
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import bigslice_amd as bs  # noqa: E402
from bigslice_amd.frame import BytesColumn, SegmentedColumn  # noqa: E402
from bigslice_amd.schema import BYTES, Schema  # noqa: E402

DEV = "cuda:0"
SWITCH = "BIGSLICE_COGROUP_BYTES"
_DATA = {}
_SCHEMAS = {
    "word": Schema([BYTES, torch.int64], 1),
    "word_doc": Schema([BYTES, torch.int64, torch.int64], 2),
    "int64": Schema([torch.int64, torch.int64], 1),
}


def build(nshard, shape):
    def side(name):
        def gen(shard, ctx):
            yield _DATA[(name, shape, shard)]
        return bs.ReaderFunc(nshard, gen, _SCHEMAS[shape])
    return bs.Cogroup(side("a"), side("b"))


FV = bs.func(build)


def canon(frames, nkey):
    """The result in one CPU form that keeps the key order: per key
    column the keys as they come, frame after frame, then per value
    column the group lengths and the values sorted inside every group."""
    keys = [[] for _ in range(nkey)]
    nval = frames[0].num_columns - nkey
    lens = [[] for _ in range(nval)]
    flat = [[] for _ in range(nval)]
    for f in frames:
        for c in range(nkey):
            k = f.columns[c]
            if isinstance(k, BytesColumn):
                keys[c].extend(k.tolists())
            elif isinstance(k, torch.Tensor):
                keys[c].extend(k.cpu().tolist())
            else:
                keys[c].extend(k)
        for vi, col in enumerate(f.columns[nkey:]):
            if isinstance(col, SegmentedColumn):
                s, e = col.starts.cpu(), col.ends.cpu()
                ln = e - s
                first = torch.cumsum(ln, 0) - ln
                idx = (torch.repeat_interleave(s - first, ln)
                       + torch.arange(int(ln.sum())))
                lens[vi].append(ln)
                flat[vi].append(col.values.cpu()[idx])
            else:
                lens[vi].append(torch.tensor([len(x) for x in col],
                                             dtype=torch.int64))
                flat[vi].append(torch.tensor(
                    list(itertools.chain.from_iterable(col)),
                    dtype=torch.int64))
    out = list(keys)
    for vi in range(nval):
        ln, v = torch.cat(lens[vi]), torch.cat(flat[vi])
        gid = torch.repeat_interleave(torch.arange(ln.shape[0]), ln)
        o = torch.sort(v, stable=True).indices
        o = o[torch.sort(gid[o], stable=True).indices]
        out += [ln, v[o]]
    return out


def same(a, b):
    return len(a) == len(b) and all(
        torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y
        for x, y in zip(a, b))


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def once(sess, nshard, shape, switch):
    os.environ[SWITCH] = switch
    sync()
    t0 = time.perf_counter()
    res = sess.run(FV, nshard, shape)
    res.discard()
    sync()
    return (time.perf_counter() - t0) * 1000


def result(sess, nshard, shape, switch):
    os.environ[SWITCH] = switch
    res = sess.run(FV, nshard, shape)
    frames = [f for f in res.open() if len(f)]
    out = canon(frames, _SCHEMAS[shape].prefix)
    res.discard()
    return out


def mmm(ts):
    return [round(min(ts), 3), round(statistics.median(ts), 3),
            round(max(ts), 3)]


def rank_cost(words, nshard, reps=5):
    """The byte-order ranks of one shard's share of the vocabulary, on
    their own: (ms per call: min/median/max, refinement rounds)."""
    from bigslice_amd.kernels import bytesort
    per = len(words) // nshard
    col = words[0:per]
    ids = col.ids64()
    st, ts = {}, []
    bytesort.order_ranks(col, ids=ids, stats=st)
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        bytesort.order_ranks(col, ids=ids)
        sync()
        ts.append((time.perf_counter() - t0) * 1000)
    return per, mmm(ts), st.get("rounds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1 << 22,
                    help="rows per side")
    ap.add_argument("--vocab", type=int, default=1 << 20)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--device", default=DEV)
    ap.add_argument("--device-only", action="store_true",
                    help="time the device arms alone (for a kernel "
                         "trace); the arms are still checked equal")
    args = ap.parse_args()
    assert args.runs >= 5 or args.device_only, \
        "at least five interleaved runs per arm"
    dev, nshard = args.device, args.shards
    g = torch.Generator(device=dev)
    g.manual_seed(24)
    per = args.rows // nshard
    docs = 16
    words = BytesColumn.from_list(
        [b"term-%d" % i for i in range(args.vocab)], dev)

    def rnd(hi):
        return torch.randint(0, hi, (per,), dtype=torch.int64, device=dev,
                             generator=g)
    for name in ("a", "b"):
        for s in range(nshard):
            w, w2, d, v = (rnd(args.vocab), rnd(args.vocab // docs),
                           rnd(docs), rnd(1 << 30))
            _DATA[(name, "word", s)] = (words.gather(w), v)
            _DATA[(name, "word_doc", s)] = (words.gather(w2), d, v)
            _DATA[(name, "int64", s)] = (w, v)
    sess = bs.start(parallelism=nshard, device=dev)
    groups = {}
    for shape in ("word", "word_doc"):
        want = result(sess, nshard, shape, "0")
        got = result(sess, nshard, shape, "1")
        assert same(want, got), "arms differ on " + shape
        groups[shape] = len(want[0])
        del want, got
        print("arms agree on %d %s keys, in order"
              % (groups[shape], shape), file=sys.stderr, flush=True)
    for shape in ("word", "word_doc", "int64"):  # warm the allocator
        once(sess, nshard, shape, "1")
    host = {"word": [], "word_doc": []}
    devt = {"word": [], "word_doc": [], "int64": []}
    for i in range(args.runs):
        for shape in ("word", "word_doc"):
            if not args.device_only:
                host[shape].append(once(sess, nshard, shape, "0"))
            devt[shape].append(once(sess, nshard, shape, "1"))
        devt["int64"].append(once(sess, nshard, "int64", "1"))
        print("run %d: " % i + ", ".join(
            "%s host %.0f ms device %.2f ms" % (
                s, host[s][-1] if host[s] else float("nan"), devt[s][-1])
            for s in ("word", "word_doc"))
            + ", int64 device %.2f ms" % devt["int64"][-1],
            file=sys.stderr, flush=True)
    os.environ.pop(SWITCH, None)
    sess.shutdown()
    rank_rows, rank_ms, rounds = rank_cost(words, nshard)
    rec = {
        "rows_per_side": per * nshard, "vocab": args.vocab,
        "keys": groups, "shards": nshard, "runs": args.runs, "device": dev,
        "single_int64_key_device_ms": [round(x, 3) for x in devt["int64"]],
        "single_int64_key_min_med_max": mmm(devt["int64"]),
        "order_ranks_rows": rank_rows,
        "order_ranks_ms_min_med_max": rank_ms,
        "refinement_rounds": rounds,
    }
    one = statistics.median(devt["int64"])
    for shape in ("word", "word_doc"):
        rec[shape + "_device_ms"] = [round(x, 3) for x in devt[shape]]
        rec[shape + "_device_min_med_max"] = mmm(devt[shape])
        rec[shape + "_over_single_int64_median"] = round(
            statistics.median(devt[shape]) / one, 2)
        if host[shape]:
            rec[shape + "_host_ms"] = [round(x, 3) for x in host[shape]]
            rec[shape + "_host_min_med_max"] = mmm(host[shape])
            rec[shape + "_device_slowest_below_host_fastest"] = (
                max(devt[shape]) < min(host[shape]))
            rec[shape + "_host_over_device_median"] = round(
                statistics.median(host[shape])
                / statistics.median(devt[shape]), 1)
    print(json.dumps(rec), flush=True)
    print("rows/side %d, vocabulary %d, %d shards, ms min/med/max" % (
        per * nshard, args.vocab, nshard))
    for shape in ("word", "word_doc"):
        if host[shape]:
            print("  %-28s %s" % (shape + " host (switch off)", " / ".join(
                "%.2f" % x for x in rec[shape + "_host_min_med_max"])))
        print("  %-28s %s" % (shape + " device", " / ".join(
            "%.2f" % x for x in rec[shape + "_device_min_med_max"])))
    print("  %-28s %s" % ("single int64 key, device", " / ".join(
        "%.2f" % x for x in rec["single_int64_key_min_med_max"])))
    print("  order_ranks of %d words: %s ms, %s rounds" % (
        rank_rows, " / ".join("%.2f" % x for x in rank_ms), rounds))


if __name__ == "__main__":
    main()
