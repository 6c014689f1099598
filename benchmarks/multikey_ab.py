"""A/B: group-by over a multi-column integer key, the lexicographic
sort path (ops/aggregate._combine_once, what TensorAggregator ran for
such keys before K21 and still runs under BIGSLICE_GB_MULTIKEY=0)
against the device hash table (kernels.MultiKeyTable).

One process, the same device tensors for both arms, runs interleaved.
Every shape is 16M rows fed as two 8M batches with one int64 sum column.
The sort arm concatenates the two batches and combines once, as
TensorAggregator does below COMBINER_TARGET_KEYS rows; the table arm
inserts each batch and finishes (compaction and its one readback
included).  Both arms must give equal results before anything is timed.

    python benchmarks/multikey_ab.py [--runs 7] [--rows 16777216]

Prints one JSON line per shape and a summary table.  The bar is at the
first shape: the table's slowest run below the sort path's fastest.
"""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from bigslice_amd.kernels import MultiKeyTable  # noqa: E402
from bigslice_amd.ops.aggregate import Aggregation, _combine_once  # noqa: E402

DEV = "cuda:0"
AGG = Aggregation(["sum"])


def shapes(rows, g):
    def rnd(hi):
        return torch.randint(0, hi, (rows,), dtype=torch.int64, device=DEV,
                             generator=g)
    yield "2col_1M", [rnd(1024), rnd(1024)]
    yield "3col_1M", [rnd(101), rnd(101), rnd(101)]
    yield "2col_64", [rnd(8), rnd(8)]
    ids = torch.randperm(rows, device=DEV, generator=g)
    yield "2col_distinct", [ids // 4096, ids % 4096]


def sort_arm(batches):
    kc = [torch.cat(c) for c in zip(*(k for k, _ in batches))]
    vc = [torch.cat(c) for c in zip(*(v for _, v in batches))]
    return _combine_once(kc, vc, AGG)


def table_arm(batches):
    t = MultiKeyTable(len(batches[0][0]), [torch.int64], ["sum"], DEV,
                      fallback=lambda k, v: _combine_once(k, v, AGG))
    for k, v in batches:
        t.insert(k, v)
    return t.finish()


def lexsorted(keys, vals):
    perm = torch.arange(keys[0].shape[0], device=keys[0].device)
    for kc in reversed(keys):
        perm = perm[torch.sort(kc[perm], stable=True).indices]
    return [c[perm] for c in list(keys) + list(vals)]


def once(fn, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(batches)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1 << 24)
    args = ap.parse_args()
    assert args.runs >= 5, "at least five interleaved runs per arm"
    g = torch.Generator(device=DEV)
    g.manual_seed(21)
    table = []
    for name, keys in shapes(args.rows, g):
        vals = torch.randint(-1000, 1000, (args.rows,), dtype=torch.int64,
                             device=DEV, generator=g)
        half = args.rows // 2
        batches = [([k[:half].contiguous() for k in keys],
                    [vals[:half].contiguous()]),
                   ([k[half:].contiguous() for k in keys],
                    [vals[half:].contiguous()])]
        del keys, vals
        want = lexsorted(*sort_arm(batches))
        got = lexsorted(*table_arm(batches))
        assert len(want) == len(got) and all(
            torch.equal(a, b) for a, b in zip(want, got)), name
        groups = int(want[0].shape[0])
        del want, got
        for fn in (sort_arm, table_arm):  # warm the allocator for both
            once(fn, batches)
        ts, tt = [], []
        for _ in range(args.runs):
            ts.append(once(sort_arm, batches))
            tt.append(once(table_arm, batches))
        ncols = len(batches[0][0])
        rec = {
            "shape": name, "rows": args.rows, "key_cols": ncols,
            "groups": groups, "runs": args.runs,
            "sort_ms": [round(x, 3) for x in ts],
            "table_ms": [round(x, 3) for x in tt],
            "sort_min_med_max": [round(min(ts), 3),
                                 round(statistics.median(ts), 3),
                                 round(max(ts), 3)],
            "table_min_med_max": [round(min(tt), 3),
                                  round(statistics.median(tt), 3),
                                  round(max(tt), 3)],
            "table_slowest_below_sort_fastest": max(tt) < min(ts),
            # end to end, compaction included: one atomic per row, and
            # 8K+4 bytes per row streamed twice plus the value column
            "table_grows_per_s": round(
                args.rows / statistics.median(tt) / 1e6, 3),
            "table_stream_gb_per_s": round(
                args.rows * (2 * (8 * ncols + 4) + 8)
                / statistics.median(tt) / 1e6, 1),
        }
        print(json.dumps(rec), flush=True)
        table.append(rec)
        del batches
        torch.cuda.empty_cache()
    print("%-14s %8s  %-26s %-26s %s" % (
        "shape", "groups", "sort min/med/max ms", "table min/med/max ms",
        "table max < sort min"))
    for r in table:
        print("%-14s %8d  %-26s %-26s %s" % (
            r["shape"], r["groups"],
            "/".join("%.2f" % x for x in r["sort_min_med_max"]),
            "/".join("%.2f" % x for x in r["table_min_med_max"]),
            r["table_slowest_below_sort_fastest"]))


if __name__ == "__main__":
    main()
