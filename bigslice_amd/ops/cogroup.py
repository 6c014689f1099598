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
  Keys with BYTES columns (K24) group by the 64-bit ids of the strings
  through those same steps, and the distinct keys of the union are then
  put into byte order by BytesColumn.order_ranks().
"""

from __future__ import annotations

import os
from typing import List

import torch

from ..frame import Frame, SegmentedColumn
from ..schema import BYTES, OBJECT, Schema, common_key_schema
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
        self._device_shape = self._device_shape_ok()

    def reader(self, shard, dep_readers, ctx: TaskContext) -> Reader:
        nkey = self.schema.prefix
        val_counts = self._val_counts
        # Device fast path: sort-merge cogroup on device with
        # SegmentedColumn outputs.
        if ctx.device != "cpu" and self._device_eligible():
            return IterReader(self._device_gen(dep_readers, ctx))

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

    def _device_shape_ok(self) -> bool:
        """Shapes the device path takes.  One key column: int64, and no
        OBJECT column in any dep.  A composite key (K22): int64/int32
        key columns (at most MAX_KEY_COLS, checked with the extension's
        constant when the reader is made) and dense torch columns
        otherwise.  A key with BYTES columns (K24): 1 to MAX_KEY_COLS
        key columns, at least one of them BYTES and the others
        int64/int32, and dense torch value columns."""
        nkey = self.schema.prefix
        dep_dts = [d.slice.schema.dtypes for d in self.deps]
        if any(dt == BYTES for dts in dep_dts for dt in dts[:nkey]):
            return all(
                any(dt == BYTES for dt in dts[:nkey])
                and all(dt == BYTES or dt in (torch.int64, torch.int32)
                        for dt in dts[:nkey])
                and all(isinstance(dt, torch.dtype) for dt in dts[nkey:])
                for dts in dep_dts)
        if nkey == 1:
            return (dep_dts[0][0] == torch.int64
                    and all(dt != OBJECT for dts in dep_dts for dt in dts))
        return all(
            all(dt in (torch.int64, torch.int32) for dt in dts[:nkey])
            and all(isinstance(dt, torch.dtype) for dt in dts[nkey:])
            for dts in dep_dts)

    def _device_eligible(self) -> bool:
        """Whether a GPU session's reader takes the device path: the
        shape fits and, for a composite key, BIGSLICE_COGROUP_MULTIKEY is
        not 0 and the extension is there (missing, it is an error unless
        the eager fallback is allowed; then the host path runs).  A
        single key costs its reader nothing here: its eight shards share
        the interpreter and the path is host-bound on small inputs.  A
        key with BYTES columns, of any width, is under
        BIGSLICE_COGROUP_BYTES in the same way."""
        from .. import kernels
        from ..kernels.groupby_multi import MAX_KEY_COLS
        if self._device_shape and self._bytes_key_cols():
            if os.environ.get("BIGSLICE_COGROUP_BYTES", "1") == "0":
                return False
            return (self.schema.prefix <= MAX_KEY_COLS
                    and kernels.native(True, "cogroup over bytes keys"))
        if not self._device_shape or self.schema.prefix == 1:
            return self._device_shape
        if os.environ.get("BIGSLICE_COGROUP_MULTIKEY", "1") == "0":
            return False
        return (self.schema.prefix <= MAX_KEY_COLS
                and kernels.native(True, "cogroup over multi-column keys"))

    def _bytes_key_cols(self) -> List[int]:
        """The BYTES columns of the key prefix."""
        return [c for c, dt in enumerate(
            self.schema.dtypes[:self.schema.prefix]) if dt == BYTES]

    def _device_gen(self, dep_readers, ctx):
        """Sort-merge cogroup over a key of nkey integer columns."""
        from ..kernels import sortedkeys as sk
        from ..sortio import sort_frame

        if self._bytes_key_cols():
            yield from self._device_gen_bytes(dep_readers, ctx)
            return
        device = ctx.device
        nkey = self.schema.prefix
        # 1. sort each dep side by key once.  One key column: the direct
        # (key, value) radix sort for one 8-byte value column, a radix
        # argsort and a gather otherwise; tuples: lexicographically.
        def by_key(f):
            if nkey == 1:
                return sort_frame(f)
            return f.select(sk.lex_argsort(f.columns[:nkey]))
        sorted_deps = []
        for r in dep_readers:
            frames = [f for f in r if len(f)]
            # (the concatenation is not kept: it is as large as the dep)
            sorted_deps.append(by_key(Frame.concat(frames))
                               if frames else None)
        dep_runs = [(sk.runs_multi(sd.columns[:nkey]) if sd is not None
                     else None) for sd in sorted_deps]
        uniq_tuples = [r[0] for r in dep_runs if r is not None]
        if not uniq_tuples:
            return
        # 2. sorted-unique union of the per-dep DISTINCT keys (tiny next
        # to the row counts); a sort only with three or more deps
        if len(uniq_tuples) == 1:
            union_cols = uniq_tuples[0]
        elif len(uniq_tuples) == 2:
            union_cols = sk.merge_sorted_unique_multi(*uniq_tuples)
        else:
            union_cols = sk.unique_sorted_multi(sk.lex_sort_keys(
                [torch.cat(cs) for cs in zip(*uniq_tuples)]))
        # 3. per-dep segments over the sorted values
        u = union_cols[0].shape[0]
        out_cols = list(union_cols)
        for di, sd in enumerate(sorted_deps):
            if sd is not None:
                out_cols.extend(_segments_for(
                    dep_runs[di], sd.columns[nkey:], union_cols,
                    sk.lex_searchsorted))
            else:
                empty_vals = [
                    torch.empty(0, dtype=dt, device=device)
                    for dt in self.deps[di].slice.schema.dtypes[nkey:]]
                zeros = torch.zeros(u, dtype=torch.int64, device=device)
                out_cols.extend(SegmentedColumn(ev, zeros, zeros)
                                for ev in empty_vals)
        frame = Frame(out_cols, prefix=nkey)
        for off in range(0, len(frame), ctx.chunk):
            yield frame.slice(off, min(off + ctx.chunk, len(frame)))

    def _device_gen_bytes(self, dep_readers, ctx):
        """Sort-merge cogroup over a key with BYTES columns (K24).  Rows
        group by id tuples — every BYTES key column stands in as its
        ids64() — through the K22 steps; one exemplar string per
        distinct tuple is carried along, and the union's tuples, few
        next to the rows, are put into byte order at the end.  The keys
        come back in the host path's order: ascending, BYTES columns as
        bytes.__lt__ orders them.  Grouping is by id: exact up to the
        2^-64-per-pair collision BytesColumn documents."""
        from ..frame import BytesColumn
        from ..kernels import bytesort
        from ..kernels import sortedkeys as sk
        from ..utils import stats

        stats.DEFAULT.add("cogroup/bytes_device", 1)
        device = ctx.device
        nkey = self.schema.prefix
        bcols = self._bytes_key_cols()
        # 1. per dep: sort a permutation by id tuple; move the value
        # columns by it, never the strings of every row
        dep_runs, dep_vals, dep_ex = [], [], []
        for r in dep_readers:
            frames = [f for f in r if len(f)]
            if not frames:
                dep_runs.append(None)
                dep_vals.append(None)
                dep_ex.append(None)
                continue
            f = Frame.concat(frames)
            idcols = [c.ids64() if isinstance(c, BytesColumn) else c
                      for c in f.columns[:nkey]]
            perm = sk.lex_argsort(idcols)
            run = sk.runs_multi([c[perm] for c in idcols])
            dep_runs.append(run)
            dep_vals.append([v[perm] for v in f.columns[nkey:]])
            # one exemplar string per run
            first = perm[run[1]]
            dep_ex.append([f.columns[c].gather(first) for c in bcols])
        uniq_tuples = [r[0] for r in dep_runs if r is not None]
        if not uniq_tuples:
            return
        # 2. sorted-unique union of the per-dep distinct id tuples
        if len(uniq_tuples) == 1:
            union_cols = uniq_tuples[0]
        elif len(uniq_tuples) == 2:
            union_cols = sk.merge_sorted_unique_multi(*uniq_tuples)
        else:
            union_cols = sk.unique_sorted_multi(sk.lex_sort_keys(
                [torch.cat(cs) for cs in zip(*uniq_tuples)]))
        u = union_cols[0].shape[0]
        # 3. per-dep segments, and for every union tuple the row of one
        # exemplar among the deps' exemplars laid end to end; both from
        # one search of the dep's tuples in the union
        src = torch.zeros(u, dtype=torch.int64, device=device)
        seg_cols = []
        base = 0
        for di, run in enumerate(dep_runs):
            if run is None:
                empty_vals = [
                    torch.empty(0, dtype=dt, device=device)
                    for dt in self.deps[di].slice.schema.dtypes[nkey:]]
                zeros = torch.zeros(u, dtype=torch.int64, device=device)
                seg_cols.extend(SegmentedColumn(ev, zeros, zeros)
                                for ev in empty_vals)
                continue
            nu = run[0][0].shape[0]
            own = torch.arange(base, base + nu, dtype=torch.int64,
                               device=device)
            idx = (sk.lex_searchsorted(union_cols, run[0])
                   if nu != u else None)
            if idx is None:
                src = own
            else:
                src[idx] = own
            seg_cols.extend(_segments_for(run, dep_vals[di], union_cols,
                                          sk.lex_searchsorted, idx=idx))
            base += nu
        have = [ex for ex in dep_ex if ex is not None]
        # 4. byte order: ranks of the union's strings, then one
        # lexicographic sort of (rank or integer column, ...)
        sort_cols = list(union_cols)
        exemplars = {}
        for bi, c in enumerate(bcols):
            ex = _concat_bytes([e[bi] for e in have]).gather(src)
            exemplars[c] = ex
            sort_cols[c] = bytesort.order_ranks(ex, ids=union_cols[c])
        perm = sk.lex_argsort(sort_cols)
        # 5. the output frame, selected once
        out_cols = [exemplars[c].gather(perm) if c in exemplars
                    else union_cols[c][perm] for c in range(nkey)]
        out_cols.extend(sc.select(perm) for sc in seg_cols)
        frame = Frame(out_cols, prefix=nkey)
        for off in range(0, len(frame), ctx.chunk):
            yield frame.slice(off, min(off + ctx.chunk, len(frame)))


def _concat_bytes(cols):
    """BytesColumns laid end to end."""
    if len(cols) == 1:
        return cols[0]
    return Frame.concat([Frame([c], 1) for c in cols]).columns[0]


def _key_sort(k):
    return k


def _segments_for(run, value_cols, union_cols, search, idx=None):
    """Per-value-column SegmentedColumns aligned with the union's key
    tuples, built from the dep's precomputed runs; search is
    sortedkeys.lex_searchsorted, idx its result for the dep's tuples
    when the caller has it.  Keys the dep lacks get (0, 0) = empty
    segments."""
    uniq_cols, starts, ends = run
    u = union_cols[0].shape[0]
    if uniq_cols[0].shape[0] != u:
        # uniq is a subset of union of equal sortedness; sizes equal
        # implies identical key sets, so scatter only when they differ
        dev = union_cols[0].device
        if idx is None:
            idx = search(union_cols, uniq_cols)
        s = torch.zeros(u, dtype=torch.int64, device=dev)
        e = torch.zeros(u, dtype=torch.int64, device=dev)
        s[idx] = starts
        e[idx] = ends
        starts, ends = s, e
    return [SegmentedColumn(v.contiguous(), starts, ends)
            for v in value_cols]
