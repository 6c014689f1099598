"""Flagship benchmark: whole-node Reshuffle+Reduce group-by-sum.

BASELINE.json north-star config 3: group-by-sum over 1B int64 rows in 8
shards (1B at 8 GPUs; per-GPU rows fixed -> weak scaling).  Each step runs
the full engine pipeline on pre-generated synthetic device data: the
adaptive producer-side combine (LDS-tier hash insert / streaming global
insert / radix-sort+reduce-by-key, chosen from a sampled key
cardinality: K9/K10/K16), the fused hash+scatter partitioner (K4),
RCCL all-to-allv over xGMI at N>1, and the consumer-side final
aggregate (pre-combined passthrough at N=1).

A plain run sets up, warms up, times --steps steps and prints one JSON
result line.  --dump-outputs DIR additionally writes the last timed
step's result (keys.npy, sums.npy; rows ordered by key, float64).
--full is reserved for secondary measurements and checks; this benchmark
has none (they live in benchmarks/), so it changes nothing today.

Usage:
  python bench.py --gpus 1 --steps 5 --warmup 2
  python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs out/
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
      --master-addr 127.0.0.1 bench.py --gpus 8 --steps 5 --warmup 2
"""

import argparse
import json
import os
import time

import numpy as np
import torch

import bigslice_amd as bs

DEFAULT_ROWS_PER_GPU = 125_000_000
DEFAULT_NKEYS = 1_000_000
DEFAULT_SHARDS = 8

DUMP_MAX_BYTES = 64 << 20
DUMP_SAMPLE_SEED = 0xD0E5

_DATA = {}


def gen_shard_data(shard, rows, nkeys, device):
    g = torch.Generator(device=device)
    g.manual_seed(0xB165 + shard)
    keys = torch.randint(0, nkeys, (rows,), dtype=torch.int64,
                         device=device, generator=g)
    vals = torch.ones(rows, dtype=torch.int64, device=device)
    return keys, vals


def build_groupby(nshard):
    def gen(shard, ctx):
        keys, vals = _DATA[shard]
        chunk = ctx.chunk
        for off in range(0, keys.shape[0], chunk):
            yield (keys[off:off + chunk], vals[off:off + chunk])
    src = bs.ReaderFunc(nshard, gen, bs.schema_of(int, int))
    return bs.Reduce(src, "sum")


groupby_func = bs.func(build_groupby)


def collect_output(res):
    """Host copy of a result's (keys, sums) columns.  Collective at N>1
    (rank 0 receives all rows, other ranks none)."""
    keys, sums = [], []
    for f in res.open():
        keys.append(f.columns[0].cpu())
        sums.append(f.columns[1].cpu())
    if not keys:
        z = torch.empty(0, dtype=torch.int64)
        return z, z
    return torch.cat(keys), torch.cat(sums)


def dump_outputs(path, keys, sums):
    """Write the group-by result as path/keys.npy and path/sums.npy
    (float64; exact, both columns are far below 2**53).  Shard and
    hash-table order is not part of the result, so rows are ordered by
    key.  An output above DUMP_MAX_BYTES is cut to a fixed seeded sample
    of those rows."""
    order = torch.argsort(keys)
    k = keys[order].numpy().astype(np.float64)
    v = sums[order].numpy().astype(np.float64)
    max_rows = DUMP_MAX_BYTES // (2 * 8)
    if k.shape[0] > max_rows:
        rs = np.random.RandomState(DUMP_SAMPLE_SEED)
        pick = np.sort(rs.choice(k.shape[0], max_rows, replace=False))
        k, v = k[pick], v[pick]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "keys.npy"), k)
    np.save(os.path.join(path, "sums.npy"), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows-per-gpu", type=int, default=DEFAULT_ROWS_PER_GPU)
    ap.add_argument("--nkeys", type=int, default=DEFAULT_NKEYS)
    ap.add_argument("--shards", type=int, default=DEFAULT_SHARDS)
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--trace", type=str, default=None,
                    help="write a Chrome trace of the run to this path")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="write the last timed step's result to "
                         "DIR/keys.npy and DIR/sums.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run secondary measurements and checks "
                         "(none here: they are separate scripts under "
                         "benchmarks/)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    distributed = world > 1
    if distributed:
        sess = bs.start(distributed=True, device=args.device,
                        trace_path=args.trace)
        device = sess.executor.device
        comm = sess.executor.comm
    else:
        device = args.device or (
            "cuda:0" if torch.cuda.is_available() else "cpu")
        sess = bs.start(parallelism=args.shards, device=device,
                        trace_path=args.trace)
        comm = None

    on_gpu = device.startswith("cuda")
    if on_gpu:
        from bigslice_amd import kernels
        assert kernels.have_extension(), \
            "HIP extension missing: build with setup.py build_ext --inplace"

    nshard = args.shards
    total_rows = args.rows_per_gpu * world
    rows_per_shard = total_rows // nshard

    # Pre-generate synthetic input for the shards this rank owns.
    for shard in range(nshard):
        if shard % world == rank:
            _DATA[shard] = gen_shard_data(shard, rows_per_shard,
                                          args.nkeys, device)

    def step(keep=False):
        res = sess.run(groupby_func, nshard)
        if keep:
            return res
        res.discard()

    def sync():
        if on_gpu:
            torch.cuda.synchronize()
        if comm is not None:
            comm.barrier()

    for _ in range(args.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps - 1):
        step()
    # With --dump-outputs the last step's result outlives the timing.
    last = step(keep=args.dump_outputs is not None)
    sync()
    elapsed = time.perf_counter() - t0

    if last is not None:
        out_keys, out_sums = collect_output(last)
        last.discard()
        if rank == 0:
            dump_outputs(args.dump_outputs, out_keys, out_sums)

    # Max over ranks (whole-job time).
    if comm is not None:
        t = torch.tensor([elapsed], dtype=torch.float64)
        if comm.backend == "nccl":
            t = t.to(device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.cpu().item())

    ms_per_step = elapsed * 1000.0 / args.steps
    rows_per_sec = (rows_per_shard * nshard) / (ms_per_step / 1000.0)

    if args.trace:
        sess.shutdown()
    if rank == 0:
        out = {
            "metric": "rows/sec (whole node) Reshuffle+Reduce group-by",
            "value": rows_per_sec,
            "unit": "rows/sec",
            "n_gpus": world if distributed else 1,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int64",
            "data": "synthetic",
            "config": {
                "model": "Reshuffle+Reduce group-by-sum (BASELINE config 3)",
                "rows_total": rows_per_shard * nshard,
                "rows_per_gpu": args.rows_per_gpu,
                "distinct_keys": args.nkeys,
                "global_batch": rows_per_shard * nshard,
                "seq_len": None,
                "shards": nshard,
                "parallelism": f"dp{world}",
                "device": device,
            },
        }
        print(json.dumps(out), flush=True)
    if distributed:
        # Clean teardown: ranks exiting at different times with a live
        # process group can SIGABRT in the backend's helper threads.
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        import traceback
        traceback.print_exc()
        raise
