"""Cogroup: co-grouped join of n slices sharing key-prefix types.

Role-parity: cogroup.go:46-272 — each input gets a shuffle dep; the reader
gathers equal-key row groups into list-valued columns.

Two paths:
* host path (object keys / small data): dict-of-lists grouping, emitting
  OBJECT list columns — exact reference semantics (Slice<k..., []v...>).
* device path (numeric single-key inputs): sort + merge by key on device;
  grouped values surface as list columns on readback.  The heavy join work
  (sort, boundary detection) runs in HIP/rocPRIM via frame sort kernels.
  Keys of 2 to 8 int64/int32 columns take the same steps over tuples
  (K22): lexicographic sort, tuple run boundaries, tuple searchsorted.
"""

from __future__ import annotations

import os
from typing import List

from ..frame import Frame
from ..schema import OBJECT, Schema, common_key_schema
from ..sliceio import IterReader, Reader
from .slice_base import Dep, Name, Slice, TaskContext


class Cogroup(Slice):
    def __init__(self, *slices: Slice):
        if not slices:
            raise TypeError("Cogroup of no slices")
        key_dts = common_key_schema([s.schema for s in slices])
        nkey = len(key_dts)
        if nkey == 0:
            raise TypeError("Cogroup requires keyed slices")
        # output: key cols, then one OBJECT (list-valued) column per
        # value column of each input (cogroup.go:94-110).
        out_dts = list(key_dts)
        self._val_counts: List[int] = []
        for s in slices:
            nv = s.schema.num_columns - s.schema.prefix
            self._val_counts.append(nv)
            out_dts.extend([OBJECT] * nv)
        num_shards = max(s.num_shards for s in slices)
        super().__init__(
            Schema(out_dts, nkey), num_shards,
            deps=[Dep(s, shuffle=True) for s in slices],
            name=Name("cogroup"))

    def reader(self, shard, dep_readers, ctx: TaskContext) -> Reader:
        nkey = self.schema.prefix
        val_counts = self._val_counts
        # Device fast path: single int64 key, numeric value columns ->
        # sort-merge cogroup on device with SegmentedColumn outputs.
        import torch as _t
        if (ctx.device != "cpu" and nkey == 1
                and self.deps[0].slice.schema.dtypes[0] == _t.int64
                and all(dt != OBJECT
                        for d in self.deps for dt in d.slice.schema.dtypes)):
            return IterReader(self._device_gen(dep_readers, ctx))
        # Same path over a composite integer key (K22): lexicographic
        # sort, tuple run boundaries and a tuple searchsorted.
        # BIGSLICE_COGROUP_MULTIKEY=0 keeps such keys on the host path.
        if (ctx.device != "cpu"
                and os.environ.get("BIGSLICE_COGROUP_MULTIKEY", "1") != "0"
                and self._multikey_eligible()):
            return IterReader(self._device_multi_gen(dep_readers, ctx))

        def gen():
            # Group each dep by key on the host: key -> [lists per column]
            groups = {}  # key -> list over deps of list-of-value-tuples
            ndeps = len(dep_readers)
            for di, r in enumerate(dep_readers):
                for f in r:
                    lists = f.column_lists()
                    keys = list(zip(*lists[:nkey])) if nkey > 1 else lists[0]
                    vals = lists[nkey:]
                    for i, k in enumerate(keys):
                        g = groups.get(k)
                        if g is None:
                            g = [[] for _ in range(ndeps)]
                            groups[k] = g
                        g[di].append(tuple(v[i] for v in vals))
            if not groups:
                return
            items = sorted(groups.items(), key=lambda kv: _key_sort(kv[0]))
            for off in range(0, len(items), ctx.chunk):
                part = items[off:off + ctx.chunk]
                if nkey > 1:
                    key_cols = [list(c) for c in
                                zip(*[k for k, _ in part])]
                else:
                    key_cols = [[k for k, _ in part]]
                out_cols: List[list] = [list(c) for c in key_cols]
                for di in range(ndeps):
                    nv = val_counts[di]
                    for vi in range(nv):
                        out_cols.append(
                            [[row[vi] for row in g[di]] for _, g in part])
                yield Frame.from_lists(out_cols, schema=self.schema)
        return IterReader(gen())

    def _multikey_eligible(self) -> bool:
        """Shapes the composite-key device path takes on a GPU session:
        2..MAX_KEY_COLS int64/int32 key columns and dense torch columns
        otherwise.  A missing extension is an error there, unless the
        eager fallback is allowed; then the host path runs."""
        import torch

        from .. import kernels
        from ..kernels.groupby_multi import MAX_KEY_COLS
        nkey = self.schema.prefix
        if not 2 <= nkey <= MAX_KEY_COLS:
            return False
        for d in self.deps:
            dts = d.slice.schema.dtypes
            if not all(dt in (torch.int64, torch.int32)
                       for dt in dts[:nkey]):
                return False
            if not all(isinstance(dt, torch.dtype) for dt in dts[nkey:]):
                return False
        if not kernels.have_extension():
            if not kernels.ALLOW_FALLBACK:
                kernels._require("cogroup over multi-column keys")
            return False
        return True


def _key_sort(k):
    return k


def _segments_for(run, value_cols, union_keys):
    """Per-value-column SegmentedColumns aligned with union_keys,
    built from the dep's precomputed runs.  Keys the dep lacks get
    (0, 0) = empty segments."""
    import torch

    from ..frame import SegmentedColumn

    uniq, starts, ends = run
    u = union_keys.shape[0]
    if uniq.shape[0] != u:
        # uniq is a subset of union of equal sortedness; sizes equal
        # implies identical key sets, so scatter only when they differ
        idx = torch.searchsorted(union_keys, uniq)
        s = torch.zeros(u, dtype=torch.int64, device=union_keys.device)
        e = torch.zeros(u, dtype=torch.int64, device=union_keys.device)
        s[idx] = starts
        e[idx] = ends
        starts, ends = s, e
    return [SegmentedColumn(v.contiguous(), starts, ends)
            for v in value_cols]


# Attach the device generator to Cogroup (kept separate for readability).
def _cogroup_device_gen(self, dep_readers, ctx):
    import torch

    from ..frame import Frame, SegmentedColumn

    from ..sortio import sort_frame
    from .. import kernels
    from ..kernels.sortedkeys import merge_sorted_unique, runs, unique_sorted

    device = ctx.device
    # 1. sort each dep side by key once (direct kv radix for 2-column)
    sorted_deps = []
    for r in dep_readers:
        frames = [f for f in r]
        sorted_deps.append(sort_frame(Frame.concat(frames))
                           if frames else None)
    dep_runs = [(runs(sd.columns[0].contiguous()) if sd is not None
                 else None) for sd in sorted_deps]
    uniq_arrays = [r[0] for r in dep_runs if r is not None]
    if not uniq_arrays:
        return
    # 2. sorted-unique union of the per-dep DISTINCT keys (tiny next
    # to the row counts); radix only as a multi-dep fallback
    if len(uniq_arrays) == 1:
        union_keys = uniq_arrays[0]
    elif len(uniq_arrays) == 2:
        union_keys = merge_sorted_unique(uniq_arrays[0], uniq_arrays[1])
    else:
        union_keys = unique_sorted(
            kernels.radix_sort_keys(torch.cat(uniq_arrays)))
    # 3. per-dep segments over the sorted values
    out_cols = [union_keys]
    for di, sd in enumerate(sorted_deps):
        if sd is not None:
            out_cols.extend(_segments_for(dep_runs[di], sd.columns[1:],
                                          union_keys))
        else:
            empty_vals = [torch.empty(0, dtype=dt, device=device)
                          for dt in self.deps[di].slice.schema.dtypes[1:]]
            zeros = torch.zeros(union_keys.shape[0], dtype=torch.int64,
                                device=device)
            out_cols.extend(SegmentedColumn(ev, zeros, zeros)
                            for ev in empty_vals)
    frame = Frame(out_cols, prefix=1)
    for off in range(0, len(frame), ctx.chunk):
        yield frame.slice(off, min(off + ctx.chunk, len(frame)))


Cogroup._device_gen = _cogroup_device_gen


def _segments_for_multi(run, value_cols, union_cols):
    """_segments_for over tuple keys: the dep's runs scatter to their
    positions among the union's tuples, found by lex_searchsorted."""
    import torch

    from ..frame import SegmentedColumn
    from ..kernels.sortedkeys import lex_searchsorted

    uniq_cols, starts, ends = run
    u = union_cols[0].shape[0]
    if uniq_cols[0].shape[0] != u:
        # a subset of the union, in the same order (see _segments_for)
        dev = union_cols[0].device
        idx = lex_searchsorted(union_cols, uniq_cols)
        s = torch.zeros(u, dtype=torch.int64, device=dev)
        e = torch.zeros(u, dtype=torch.int64, device=dev)
        s[idx] = starts
        e[idx] = ends
        starts, ends = s, e
    return [SegmentedColumn(v.contiguous(), starts, ends)
            for v in value_cols]


def _cogroup_device_multi_gen(self, dep_readers, ctx):
    """_cogroup_device_gen, step by step, for a key of nkey columns."""
    import torch

    from ..frame import Frame, SegmentedColumn
    from ..kernels.sortedkeys import (lex_argsort, merge_sorted_unique_multi,
                                      runs_multi, unique_sorted_multi)

    device = ctx.device
    nkey = self.schema.prefix
    # 1. sort each dep side lexicographically by its key columns once
    sorted_deps = []
    for r in dep_readers:
        frames = [f for f in r if len(f)]
        if not frames:
            sorted_deps.append(None)
            continue
        f = Frame.concat(frames)
        sorted_deps.append(f.select(lex_argsort(f.columns[:nkey])))
    dep_runs = [(runs_multi(sd.columns[:nkey]) if sd is not None else None)
                for sd in sorted_deps]
    uniq_tuples = [r[0] for r in dep_runs if r is not None]
    if not uniq_tuples:
        return
    # 2. sorted-unique union of the per-dep DISTINCT tuples
    if len(uniq_tuples) == 1:
        union_cols = uniq_tuples[0]
    elif len(uniq_tuples) == 2:
        union_cols = merge_sorted_unique_multi(uniq_tuples[0],
                                               uniq_tuples[1])
    else:
        cat = [torch.cat(cs) for cs in zip(*uniq_tuples)]
        perm = lex_argsort(cat)
        union_cols = unique_sorted_multi([c[perm] for c in cat])
    # 3. per-dep segments over the sorted values
    u = union_cols[0].shape[0]
    out_cols = list(union_cols)
    for di, sd in enumerate(sorted_deps):
        if sd is not None:
            out_cols.extend(_segments_for_multi(
                dep_runs[di], sd.columns[nkey:], union_cols))
        else:
            empty_vals = [torch.empty(0, dtype=dt, device=device)
                          for dt in self.deps[di].slice.schema.dtypes[nkey:]]
            zeros = torch.zeros(u, dtype=torch.int64, device=device)
            out_cols.extend(SegmentedColumn(ev, zeros, zeros)
                            for ev in empty_vals)
    frame = Frame(out_cols, prefix=nkey)
    for off in range(0, len(frame), ctx.chunk):
        yield frame.slice(off, min(off + ctx.chunk, len(frame)))


Cogroup._device_multi_gen = _cogroup_device_multi_gen
