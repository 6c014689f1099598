"""A/B: Cogroup of two slices keyed by a two-column integer tuple, the
host path (a Python dict of tuples, what every GPU session ran for such
keys before K22 and still runs under BIGSLICE_COGROUP_MULTIKEY=0)
against the device sort-merge path (lex_argsort, runs_multi,
lex_searchsorted).

One process, one session, the same device tensors for both arms, runs
interleaved.  Inputs: two slices of --rows rows each over about --tuples
distinct (a, b) tuples, one int64 value column per side.  A step is
`sess.run(...)` plus `discard()`, as benchmarks/configs.py times config
4.  Both arms must give equal results before anything is timed: equal
tuples, and per tuple and side the same multiset of values.  A third
series times the single-key device cogroup of the same row count and
distinct-key count in the same session, to state what the extra key
column costs.

    python benchmarks/cogroup_multikey_ab.py [--runs 5] [--rows 4194304]

Prints one JSON line and a summary.  The bar: the device arm's slowest
run below the host arm's fastest.
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
from bigslice_amd.frame import SegmentedColumn  # noqa: E402

DEV = "cuda:0"
SWITCH = "BIGSLICE_COGROUP_MULTIKEY"
_DATA = {}


def build(nshard, nkey):
    def side(name):
        def gen(shard, ctx):
            yield _DATA[(name, nkey, shard)]
        return bs.ReaderFunc(nshard, gen,
                             bs.schema_of(*([int] * (nkey + 1)),
                                          prefix=nkey))
    return bs.Cogroup(side("a"), side("b"))


FV = bs.func(build)


def _lexperm(cols):
    perm = torch.arange(cols[0].shape[0])
    for c in reversed(cols):
        perm = perm[torch.sort(c[perm], stable=True).indices]
    return perm


def canon(frames, nkey):
    """The result in one canonical CPU form: key columns in lexicographic
    order, then per value column the group lengths and the values sorted
    inside every group."""
    keys = [[] for _ in range(nkey)]
    nval = frames[0].num_columns - nkey
    lens = [[] for _ in range(nval)]
    flat = [[] for _ in range(nval)]
    for f in frames:
        for c in range(nkey):
            k = f.columns[c]
            keys[c].append(k.cpu() if isinstance(k, torch.Tensor)
                           else torch.tensor(list(k), dtype=torch.int64))
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
    keys = [torch.cat(k) for k in keys]
    perm = _lexperm(keys)
    rank = torch.empty_like(perm)
    rank[perm] = torch.arange(perm.shape[0])
    out = [k[perm] for k in keys]
    for vi in range(nval):
        ln, v = torch.cat(lens[vi]), torch.cat(flat[vi])
        gid = rank[torch.repeat_interleave(torch.arange(ln.shape[0]), ln)]
        o = torch.sort(v, stable=True).indices
        o = o[torch.sort(gid[o], stable=True).indices]
        out += [ln[perm], v[o]]
    return out


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def once(sess, nshard, nkey, switch):
    os.environ[SWITCH] = switch
    sync()
    t0 = time.perf_counter()
    res = sess.run(FV, nshard, nkey)
    res.discard()
    sync()
    return (time.perf_counter() - t0) * 1000


def result(sess, nshard, nkey, switch):
    os.environ[SWITCH] = switch
    res = sess.run(FV, nshard, nkey)
    frames = [f for f in res.open() if len(f)]
    out = canon(frames, nkey)
    res.discard()
    return out


def mmm(ts):
    return [round(min(ts), 3), round(statistics.median(ts), 3),
            round(max(ts), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1 << 22,
                    help="rows per side")
    ap.add_argument("--tuples", type=int, default=1 << 20)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--device", default=DEV)
    args = ap.parse_args()
    assert args.runs >= 5, "at least five interleaved runs per arm"
    dev, nshard = args.device, args.shards
    g = torch.Generator(device=dev)
    g.manual_seed(22)
    per = args.rows // nshard
    side = int(round(args.tuples ** 0.5))

    def rnd(hi):
        return torch.randint(0, hi, (per,), dtype=torch.int64, device=dev,
                             generator=g)
    for name in ("a", "b"):
        for s in range(nshard):
            k1, k2, v = rnd(side), rnd(side), rnd(1 << 30)
            _DATA[(name, 2, s)] = (k1, k2, v)
            _DATA[(name, 1, s)] = (k1 * side + k2, v)
    sess = bs.start(parallelism=nshard, device=dev)
    want = result(sess, nshard, 2, "0")
    got = result(sess, nshard, 2, "1")
    assert len(want) == len(got) and all(
        torch.equal(a, b) for a, b in zip(want, got)), "arms differ"
    groups = int(want[0].shape[0])
    del want, got
    print("arms agree on %d tuples" % groups, file=sys.stderr, flush=True)
    once(sess, nshard, 2, "1")  # warm the allocator
    once(sess, nshard, 1, "1")
    th, td, t1 = [], [], []
    for i in range(args.runs):
        th.append(once(sess, nshard, 2, "0"))
        td.append(once(sess, nshard, 2, "1"))
        t1.append(once(sess, nshard, 1, "1"))
        print("run %d: host %.1f ms, device %.2f ms, single-key %.2f ms"
              % (i, th[-1], td[-1], t1[-1]), file=sys.stderr, flush=True)
    os.environ.pop(SWITCH, None)
    sess.shutdown()
    rec = {
        "rows_per_side": per * nshard, "tuples": groups, "shards": nshard,
        "runs": args.runs, "device": dev,
        "host_ms": [round(x, 3) for x in th],
        "device_ms": [round(x, 3) for x in td],
        "single_key_device_ms": [round(x, 3) for x in t1],
        "host_min_med_max": mmm(th), "device_min_med_max": mmm(td),
        "single_key_min_med_max": mmm(t1),
        "device_slowest_below_host_fastest": max(td) < min(th),
        "host_over_device_median": round(
            statistics.median(th) / statistics.median(td), 1),
        "two_columns_over_one_median": round(
            statistics.median(td) / statistics.median(t1), 2),
    }
    print(json.dumps(rec), flush=True)
    print("rows/side %d, %d tuples, %d shards, ms min/med/max" % (
        per * nshard, groups, nshard))
    for name, key in (("host path (switch off)", "host_min_med_max"),
                      ("device path", "device_min_med_max"),
                      ("single-key device path", "single_key_min_med_max")):
        print("  %-24s %s" % (name, " / ".join("%.2f" % x for x in rec[key])))
    print("  device slowest below host fastest:",
          rec["device_slowest_below_host_fastest"])


if __name__ == "__main__":
    main()
