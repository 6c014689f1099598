"""A/B: the Map+Filter scan of BASELINE config 2 written with lambda UDFs
(eager torch ops per stage) vs with expressions (one fused kernel launch
per batch, csrc/expr.hip).  Both arms run in one process over the same
resident data, so the ratio is a same-box number.

Usage: python benchmarks/mapfilter_ab.py [--rows N] [--shards S]
                                         [--steps K] [--warmup W]
Prints one JSON line per arm (same shape as bench.py); the expression
arm adds its ratio to the lambda arm and its effective bandwidth,
(8 + 8 x survivor fraction) bytes per row over the step time.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import bigslice_amd as bs

_DATA = {}


def _source(nshard):
    def gen(shard, ctx):
        x = _DATA[shard]
        for off in range(0, x.shape[0], ctx.chunk):
            yield (x[off:off + ctx.chunk],)
    return bs.ReaderFunc(nshard, gen, bs.schema_of(int))


def build_lambda(nshard):
    mapped = bs.Map(_source(nshard), lambda x: (x * 3 + 1,))
    return bs.Filter(mapped, lambda x: (x & 7) != 0)


def build_expr(nshard):
    mapped = bs.Map(_source(nshard), bs.col(0) * 3 + 1)
    return bs.Filter(mapped, (bs.col(0) & 7) != 0)


FV = {"lambda": bs.func(build_lambda), "expr": bs.func(build_expr)}


def count_rows(res) -> int:
    """Row count from the stored frames (no row iteration)."""
    return sum(len(f) for s in range(res.num_shards)
               for f in res.reader(s, [], None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    device = "cuda:0" if torch.cuda.is_available() else "cpu"
    nshard = args.shards
    per = args.rows // nshard
    rows = per * nshard
    for s in range(nshard):
        gen = torch.Generator(device=device)
        gen.manual_seed(s)
        _DATA[s] = torch.randint(0, 1 << 40, (per,), dtype=torch.int64,
                                 device=device, generator=gen)
    sess = bs.start(parallelism=nshard, device=device)

    def sync():
        if device.startswith("cuda"):
            torch.cuda.synchronize()

    results = {}
    for arm in ("lambda", "expr"):
        res = sess.run(FV[arm], nshard)
        survivors = count_rows(res)
        res.discard()
        for _ in range(args.warmup):
            sess.run(FV[arm], nshard).discard()
        sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            sess.run(FV[arm], nshard).discard()
        sync()
        ms = (time.perf_counter() - t0) * 1000 / args.steps
        results[arm] = (ms, survivors)

    assert results["lambda"][1] == results["expr"][1], results
    for arm in ("lambda", "expr"):
        ms, survivors = results[arm]
        out = {
            "metric": f"rows/sec Map+Filter scan ({arm} UDFs)",
            "value": rows / (ms / 1000), "unit": "rows/sec", "n_gpus": 1,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "int64", "data": "synthetic",
            "survivors": survivors,
            "config": {"model": "Map+Filter scan (BASELINE config 2)",
                       "arm": arm, "rows_total": rows,
                       "global_batch": rows, "shards": nshard,
                       "parallelism": "dp1", "device": device},
        }
        if arm == "expr":
            out["speedup_vs_lambda"] = results["lambda"][0] / ms
            out["effective_bytes_per_sec"] = \
                (8 + 8 * survivors / rows) * rows / (ms / 1000)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
