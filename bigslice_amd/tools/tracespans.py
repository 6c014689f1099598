"""Serial stretches of a flagship step, from a rocprofv3 kernel trace.

  python -m bigslice_amd.tools.tracespans kernel_trace.csv

Reads the `--kernel-trace --output-format csv` file of a
`bench.py --gpus 1` run (one GroupTable per step) and prints, per step:

  a     start of the cardinality sample (first sort or k_gbs_* kernel) to
        the start of the first k_gbp_hist: the head of the step, during
        which no insert can run
  b     start of the finish (k_groupby_compact or k_gbf_count) to the end
        of its last kernel (k_part_scatter or k_gbf_write)
  idle  time inside the step with no kernel running
  span  end of the previous step's finish to the end of this one's
  ksum  summed kernel durations

all in microseconds, then the median, minimum and maximum over the steps
(without the first step, which carries the set-up).
A step ends with the last kernel of the finish.
"""

import csv
import statistics
import sys

FINISH_START = ("k_groupby_compact", "k_gbf_count")
FINISH_END = ("k_part_scatter", "k_gbf_write")


def load(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                         r["Kernel_Name"]))
    rows.sort()
    return rows


def steps_of(rows):
    steps, cur = [], []
    for r in rows:
        cur.append(r)
        if r[2].startswith(FINISH_END):
            steps.append(cur)
            cur = []
    return steps


def spans(step, prev_end):
    def first(pred):
        return next((r for r in step if pred(r[2])), None)
    hist = first(lambda n: n.startswith("k_gbp_hist"))
    samp = first(lambda n: "sort" in n.lower() or n.startswith("k_gbs"))
    fin = first(lambda n: n.startswith(FINISH_START))
    t0 = step[0][0] if prev_end is None else prev_end
    t1 = step[-1][1]
    busy, edge = 0, t0
    for st, en, _ in step:
        if en > edge:
            busy += en - max(st, edge)
            edge = en
    return {
        "a": (hist[0] - samp[0]) / 1e3 if hist and samp else None,
        "b": (t1 - fin[0]) / 1e3 if fin else None,
        "idle": (t1 - t0 - busy) / 1e3,
        "span": (t1 - t0) / 1e3,
        "ksum": sum(en - st for st, en, _ in step) / 1e3,
        "kernels": len(step),
    }


def main():
    steps = steps_of(load(sys.argv[1]))
    out, prev_end = [], None
    for s in steps:
        out.append(spans(s, prev_end))
        prev_end = s[-1][1]
        print("  ".join(f"{k}={v:.1f}" if isinstance(v, float) else f"{k}={v}"
                        for k, v in out[-1].items()))
    for name in ("a", "b", "idle", "span", "ksum"):
        v = [o[name] for o in out[1:] if o[name] is not None]
        if v:
            print(f"{name}: median {statistics.median(v):.1f} "
                  f"min {min(v):.1f} max {max(v):.1f}")


if __name__ == "__main__":
    main()
