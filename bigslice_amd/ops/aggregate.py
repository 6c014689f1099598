"""Hash aggregation: the engine's group-by-combine core.

Role-parity with the reference's combiner machinery (exec/combiner.go: the
open-addressing combiningFrame K9, two-level combine K10, spilling combiner
K11; accum.go accumulators K12).  The MI355X-native design replaces the
row-wise open-addressing table with whole-batch device aggregation:

* single numeric key column + numeric values: a HIP hash-aggregate kernel
  (csrc/groupby.hip) using an HBM open-addressing table with LDS
  pre-aggregation per workgroup; torch scatter_reduce is the portable
  fallback (and the CPU path).
* 2..8 int64/int32 key columns + numeric values: a HIP table keyed by the
  whole tuple (csrc/groupby_multi.hip); other numeric composite keys and
  the CPU path use a lexicographic sort + segment reduce.
* 2..8 key columns of which some are BYTES and the rest int64/int32, on a
  GPU: the same table over the strings' 64-bit ids, with a HIP id
  dictionary per BYTES column (csrc/iddict.hip) that keeps one exemplar
  string per id for the output.
* arbitrary keys/values/fns: a host dict accumulator (the reference's
  accum.go path).

An Aggregation names the per-value-column combine op; builtins run on
device, arbitrary callables run on host.
"""

from __future__ import annotations

import functools
import operator
import os
from typing import Callable, List, Optional, Sequence, Union

import torch

from .. import config
from ..frame import Frame
from ..schema import Schema, is_object

BUILTIN_AGGS = ("sum", "min", "max", "prod")

_CALLABLE_MAP = {
    operator.add: "sum",
    operator.mul: "prod",
    min: "min",
    max: "max",
}


def resolve_agg(fn: Union[str, Callable]) -> Union[str, Callable]:
    """Map a user combine fn to a builtin name when possible."""
    if isinstance(fn, str):
        if fn not in BUILTIN_AGGS:
            raise ValueError(f"unknown aggregation {fn!r}")
        return fn
    return _CALLABLE_MAP.get(fn, fn)


class Aggregation:
    """Per-value-column combine spec for a keyed reduce."""

    def __init__(self, aggs: Sequence[Union[str, Callable]]):
        self.aggs = [resolve_agg(a) for a in aggs]

    @property
    def all_builtin(self) -> bool:
        return all(isinstance(a, str) for a in self.aggs)

    def key(self):
        """Structural identity for compiler memoization: equal specs
        share producer tasks, different specs must not."""
        return tuple(a if isinstance(a, str) else id(a)
                     for a in self.aggs)

    @property
    def name(self) -> str:
        """Stable human label (golden graphs, traces)."""
        return "+".join(
            a if isinstance(a, str) else getattr(a, "__name__", "fn")
            for a in self.aggs)

    def __repr__(self):
        return f"Aggregation({self.aggs})"


def make_aggregator(schema: Schema, agg: Aggregation, device: str,
                    seed: int = config.COMBINER_HASH_SEED):
    """Choose the right aggregator implementation for a schema:
    tensor path for any all-numeric schema (single- or multi-column
    keys), device dictionary path for a single BYTES key, id-tuple path
    for a composite key with BYTES columns on a GPU
    (BIGSLICE_GB_BYTES_MULTIKEY=0 turns that off), host dict path for
    object keys / arbitrary combine fns."""
    from ..schema import is_bytes
    numeric = (not any(is_object(d) or is_bytes(d)
                       for d in schema.dtypes))
    if agg.all_builtin and numeric and schema.prefix >= 1:
        return TensorAggregator(schema, agg, device)
    if (agg.all_builtin and schema.prefix == 1
            and is_bytes(schema.dtypes[0])
            and not any(is_object(d) or is_bytes(d)
                        for d in schema.dtypes[1:])):
        return BytesKeyAggregator(schema, agg, device)
    from .. import kernels
    if device.startswith("cuda") and bytes_tuple_supported(schema, agg) \
            and os.environ.get("BIGSLICE_GB_BYTES_MULTIKEY", "1") != "0" \
            and kernels.native(True, "groupby"):
        return BytesTupleAggregator(schema, agg, device)
    return DictAggregator(schema, agg)


# Small device frames are concatenated before a table is touched: one set
# of launches instead of many (consumer-side shuffle buckets are ~100k
# rows).
_SMALL_ROWS = 1 << 20


class _Pending:
    """Frames waiting to go on as one."""

    def __init__(self):
        self.frames: List[Frame] = []
        self.rows = 0

    def add(self, frame: Frame) -> None:
        self.frames.append(frame)
        self.rows += len(frame)

    def take(self) -> Optional[Frame]:
        """The waiting frames as one (None without any); none wait after."""
        if not self.frames:
            return None
        f = Frame.concat(self.frames)
        self.frames.clear()
        self.rows = 0
        return f

    def flush(self, sink) -> None:
        f = self.take()
        if f is not None:
            sink(f)

    def feed(self, frame: Frame, sink) -> None:
        """A frame of _SMALL_ROWS rows or more goes to sink at once; a
        smaller one waits until four times as many rows do."""
        if len(frame) >= _SMALL_ROWS:
            sink(frame)
            return
        self.add(frame)
        if self.rows >= 4 * _SMALL_ROWS:
            self.flush(sink)


def bytes_tuple_supported(schema: Schema, agg: Aggregation) -> bool:
    """Shapes BytesTupleAggregator takes: builtin aggregations, a prefix
    of 2..MAX_KEY_COLS columns of which at least one is BYTES and the
    others int64/int32, and dense value columns MultiKeyTable accepts
    (with every BYTES key counted as its int64 id)."""
    from ..kernels import groupby_multi as gbm
    from ..schema import is_bytes
    keys = schema.dtypes[:schema.prefix]
    vals = schema.dtypes[schema.prefix:]
    if not agg.all_builtin or not any(is_bytes(d) for d in keys):
        return False
    if any(is_object(d) or is_bytes(d) for d in vals):
        return False
    if any(is_object(d) for d in keys):
        return False
    return gbm.multikey_supported(
        [torch.int64 if is_bytes(d) else d for d in keys], vals, agg.aggs)


class BytesTupleAggregator:
    """Keyed reduce over a composite key with BYTES columns (K23): 2 to
    MAX_KEY_COLS key columns, at least one BYTES, the others int64/int32.

    Every BYTES key column is replaced by its 64-bit id and the id tuples
    group through the numeric TensorAggregator (the HIP MultiKeyTable on
    a GPU, whose collision fallback is _combine_once over the id tuples).
    One IdDictionary per BYTES column (a device hash table; no sort, no
    torch.unique) keeps one exemplar string per id for the output.
    Grouping is by id: exact up to the 2^-64-per-pair id collision that
    BytesColumn documents.

    On "cpu" the dictionary runs its host mirror and the inner aggregator
    its sort path; no session routes here on the CPU, it is how the logic
    is tested without a GPU.
    """

    def __init__(self, schema: Schema, agg: Aggregation, device: str):
        from ..kernels.iddict import IdDictionary
        from ..schema import Schema as S
        from ..schema import is_bytes
        if not bytes_tuple_supported(schema, agg):
            raise ValueError("unsupported composite BYTES key shape")
        self.schema = schema
        self.nkey = schema.prefix
        self.device = device
        self.bytes_cols = [i for i in range(self.nkey)
                           if is_bytes(schema.dtypes[i])]
        inner_dts = tuple(torch.int64 if i in self.bytes_cols else dt
                          for i, dt in enumerate(schema.dtypes))
        self.inner = TensorAggregator(S(inner_dts, self.nkey), agg, device)
        self.dicts = {i: IdDictionary(device) for i in self.bytes_cols}
        # in front of the inner aggregator's: both tables see one frame
        self._pending = _Pending()

    def add(self, frame: Frame) -> None:
        if len(frame) == 0:
            return
        if frame.device != self.device:
            frame = frame.to(self.device)
        self._pending.feed(frame, self._insert)

    def _insert(self, f: Frame) -> None:
        cols = list(f.columns)
        for i in self.bytes_cols:
            ids = cols[i].ids64()
            self.dicts[i].add(ids, cols[i])
            cols[i] = ids
        self.inner.add(Frame(cols, self.nkey))

    def result_frames(self, chunk: int):
        self._pending.flush(self._insert)
        first = True
        for f in self.inner.result_frames(chunk):
            if first:
                from ..utils import stats
                stats.DEFAULT.add("combiner/bytes_tuple_tables", 1)
                first = False
            cols = list(f.columns)
            for i in self.bytes_cols:
                d = self.dicts[i]
                cols[i] = d.strings().gather(d.lookup(cols[i]))
            yield Frame(cols, self.nkey, combined_id=f.combined_id)


class BytesKeyAggregator:
    """Keyed reduce over a device varlen BYTES key: rows group by the
    key's 64-bit dictionary id through the numeric TensorAggregator
    (HIP GroupTable on GPU), while a per-aggregator dictionary maps
    each id back to one exemplar byte row for the output.  This is the
    device-resident string group-by of the reference's string ops
    (frame/ops_builtin.go:143-164); id collisions are 2^-64 per pair,
    the accepted dictionary-encoding tradeoff (see frame.BytesColumn).
    """

    def __init__(self, schema: Schema, agg: Aggregation, device: str):
        from ..schema import Schema as S
        self.schema = schema
        inner_schema = S((torch.int64,) + tuple(schema.dtypes[1:]), 1)
        self.inner = TensorAggregator(inner_schema, agg, device)
        self.device = device
        self.dict_ids: Optional[torch.Tensor] = None  # sorted
        self.dict_keys = None  # BytesColumn exemplars, id-sorted

    def add(self, frame: Frame) -> None:
        if len(frame) == 0:
            return
        key_col = frame.columns[0]
        ids = key_col.ids64()
        uniq = torch.unique(ids)
        if self.dict_ids is not None:
            new = uniq[~torch.isin(uniq, self.dict_ids)]
        else:
            new = uniq
        if new.numel():
            # exemplar row per new id: first occurrence in this frame
            sidx = torch.argsort(ids, stable=True)
            pos = torch.searchsorted(ids[sidx], new)
            exemplars = key_col.select(sidx[pos])
            if self.dict_ids is None:
                merged_ids, merged_keys = new, exemplars
            else:
                from ..frame import BytesColumn
                cat_ids = torch.cat([self.dict_ids, new])
                order = torch.argsort(cat_ids)
                merged_ids = cat_ids[order]
                both = Frame.concat([
                    Frame([self.dict_keys], 1),
                    Frame([exemplars], 1)]).columns[0]
                merged_keys = both.select(order)
            self.dict_ids = merged_ids
            self.dict_keys = merged_keys
        self.inner.add(Frame([ids] + list(frame.columns[1:]), 1))

    def result_frames(self, chunk: int):
        for f in self.inner.result_frames(chunk):
            pos = torch.searchsorted(
                self.dict_ids, f.columns[0].to(self.dict_ids.device))
            keys = self.dict_keys.select(pos)
            yield Frame([keys] + list(f.columns[1:]), 1,
                        combined_id=f.combined_id)


class TensorAggregator:
    """Device/CPU aggregation for numeric key column(s).

    Single int64 keys on GPU stream through the HIP GroupTable, and
    tuples of 2..8 int64/int32 key columns through the HIP MultiKeyTable
    (BIGSLICE_GB_MULTIKEY=0 turns that off); everything else combines
    via sort-based segment reduce (multi-column keys use a lexicographic
    sort + boundary detection).  State is re-compacted on flush,
    bounding memory at O(distinct keys).
    """

    def __init__(self, schema: Schema, agg: Aggregation, device: str):
        self.schema = schema
        self.nkey = schema.prefix
        self.agg = agg
        self.device = device
        self.keys: Optional[List[torch.Tensor]] = None
        self.vals: List[torch.Tensor] = []
        self._pending = _Pending()
        # Pre-combined passthrough: while every added frame carries the
        # SAME combiner instance id, its keys are globally unique and
        # re-aggregation is the identity (the machine-combiners
        # single-stream case, e.g. one GPU's shared combine feeding its
        # own consumer).  A frame from a different (or no) instance
        # demotes everything to normal aggregation.
        self._pt_frames: Optional[List[Frame]] = []
        self._pt_id = None
        # Device fast path: stream batches straight into the HIP table
        # of the key's width (no host sync until finish).
        self._table = None
        if device.startswith("cuda"):
            from .. import kernels
            from ..kernels import groupby_multi as gbm
            if self.nkey == 1:
                supported = kernels.groupby_shape_supported
                make = kernels.GroupTable
            else:
                def supported(*shape):
                    return (gbm.multikey_supported(*shape)
                            and gbm.Options.from_env().enabled)
                # two tuples with one fingerprint: regroup exactly
                make = functools.partial(
                    gbm.MultiKeyTable, self.nkey,
                    fallback=lambda k, v: _combine_once(k, v, self.agg))
            val_dts = schema.dtypes[self.nkey:]
            if supported(schema.dtypes[:self.nkey], val_dts, agg.aggs) \
                    and kernels.native(True, "groupby"):
                self._table = make(val_dts, agg.aggs, device)

    def add(self, frame: Frame) -> None:
        if len(frame) == 0:
            return
        if frame.device != self.device:
            frame = frame.to(self.device)
        if self._pt_frames is not None:
            cid = frame.combined_id
            if cid is not None and (self._pt_id is None
                                    or cid == self._pt_id):
                self._pt_id = cid
                self._pt_frames.append(frame)
                return
            # demote: replay buffered frames through normal aggregation
            buffered, self._pt_frames = self._pt_frames, None
            for f in buffered:
                self._add_normal(f)
        self._add_normal(frame)

    def _add_normal(self, frame: Frame) -> None:
        if self._table is not None:
            self._pending.feed(frame, self._table_insert)
            return
        self._pending.add(frame)
        if self._pending.rows >= config.COMBINER_TARGET_KEYS:
            self._flush()

    def _table_insert(self, f: Frame) -> None:
        vals = [c.contiguous() for c in f.columns[self.nkey:]]
        if self.nkey == 1:
            self._table.insert(f.columns[0].contiguous(), vals)
        else:
            self._table.insert(list(f.columns[:self.nkey]), vals)

    def _flush(self) -> None:
        f = self._pending.take()
        if f is None:
            return
        keys = [c for c in f.columns[: self.nkey]]
        vals = list(f.columns[self.nkey:])
        if self.keys is not None:
            keys = [torch.cat([sk, k]) for sk, k in zip(self.keys, keys)]
            vals = [torch.cat([sv, v]) for sv, v in zip(self.vals, vals)]
        self.keys, self.vals = _combine_once(keys, vals, self.agg)

    def result_partitions(self, nparts: int, chunk: int):
        """The result already split by the default partitioner, for a
        shuffle producer: per partition a list of frames of at most
        `chunk` rows, all with one combined_id.  Only a GroupTable gives
        that (GroupTable.finish_partitioned); None for pass-through
        frames, without a table, for a multi-column key, on a CPU and
        wherever the table declines: result_frames + split_frame then
        give the same buckets."""
        if (self._pt_frames is not None or self._table is None
                or self.nkey != 1 or not self.device.startswith("cuda")):
            return None
        self._pending.flush(self._table_insert)
        parts = self._table.finish_partitioned(nparts)
        if parts is None:
            return None
        import uuid
        cid = uuid.uuid4().int & ((1 << 63) - 1)
        return [[Frame([keys[off:off + chunk]] +
                       [v[off:off + chunk] for v in vals],
                       self.schema.prefix, combined_id=cid)
                 for off in range(0, keys.shape[0], chunk)]
                for keys, vals in parts]

    def result_frames(self, chunk: int):
        if self._pt_frames is not None:
            # single pre-combined stream: identity (keys already unique)
            for f in self._pt_frames:
                yield f
            return
        if self._table is not None:
            self._pending.flush(self._table_insert)
            keys, vals = self._table.finish()
            keys = [keys] if self.nkey == 1 else keys
            if keys[0].shape[0]:
                self.keys, self.vals = keys, vals
        else:
            self._flush()
        if self.keys is None:
            return
        import uuid
        cid = uuid.uuid4().int & ((1 << 63) - 1)
        n = self.keys[0].shape[0]
        for off in range(0, n, chunk):
            stop = min(off + chunk, n)
            yield Frame([k[off:stop] for k in self.keys] +
                        [v[off:stop] for v in self.vals],
                        self.schema.prefix, combined_id=cid)


def _combine_once(keys: List[torch.Tensor], vals: List[torch.Tensor],
                  agg: Aggregation):
    """One compaction: group rows by key column(s), combining values.

    Single-key GPU batches use the HIP hash-aggregate kernel when
    supported; otherwise a sort-based segment reduce (multi-column keys:
    lexicographic stable sort + boundary detection), which runs on both
    CPU and GPU.
    """
    from ..kernels.groupby import _AGG_CODES
    from ..kernels.sortedkeys import _SCATTER_OP
    if len(keys) == 1:
        k = keys[0]
        if k.is_cuda:
            from .. import kernels
            if kernels.groupby_supported(k, vals, agg.aggs):
                uk, ov = kernels.groupby(k, vals, agg.aggs)
                return [uk], ov
        uk, inv = torch.unique(k, return_inverse=True)
        nseg = uk.shape[0]
        uks = [uk]
    else:
        n = keys[0].shape[0]
        perm = torch.arange(n, device=keys[0].device)
        for kc in reversed(keys):
            _, o = torch.sort(kc[perm], stable=True)
            perm = perm[o]
        skeys = [kc[perm] for kc in keys]
        boundary = torch.zeros(n, dtype=torch.bool,
                               device=keys[0].device)
        boundary[0] = True
        for kc in skeys:
            boundary[1:] |= kc[1:] != kc[:-1]
        inv_sorted = boundary.cumsum(0) - 1
        nseg = int(inv_sorted[-1].item()) + 1 if n else 0
        uks = [kc[boundary] for kc in skeys]
        # map back to original row order for scatter
        inv = torch.empty(n, dtype=torch.int64, device=keys[0].device)
        inv[perm] = inv_sorted
        vals = list(vals)
    out_vals = []
    for v, a in zip(vals, agg.aggs):
        init = torch.empty(nseg, dtype=v.dtype, device=v.device)
        out = init.scatter_reduce_(
            0, inv, v, reduce=_SCATTER_OP[_AGG_CODES[a]], include_self=False)
        out_vals.append(out)
    return uks, out_vals


class DictAggregator:
    """Host dict aggregation for object keys and/or arbitrary combine fns
    (reference accum.go:28-186)."""

    def __init__(self, schema: Schema, agg: Aggregation):
        self.schema = schema
        self.agg = agg
        self.state = {}

    def add(self, frame: Frame) -> None:
        nkey = self.schema.prefix
        lists = frame.column_lists()
        keys = list(zip(*lists[:nkey])) if nkey > 1 else lists[0]
        vals = lists[nkey:]
        state = self.state
        aggs = self.agg.aggs
        if len(vals) == 1 and aggs == ["sum"]:
            vcol = vals[0]
            if isinstance(vcol, list) and vcol.count(1) == len(vcol):
                # counting shape (all-ones values): C-speed Counter
                from collections import Counter
                for k, n in Counter(keys).items():
                    cur = state.get(k)
                    if cur is None:
                        state[k] = [n]
                    else:
                        cur[0] += n
            else:
                for k, v in zip(keys, vcol):
                    cur = state.get(k)
                    if cur is None:
                        state[k] = [v]
                    else:
                        cur[0] += v
            return
        for i, k in enumerate(keys):
            row = tuple(v[i] for v in vals)
            cur = state.get(k)
            if cur is None:
                state[k] = list(row)
            else:
                for j, a in enumerate(aggs):
                    if a == "sum":
                        cur[j] += row[j]
                    elif a == "min":
                        cur[j] = min(cur[j], row[j])
                    elif a == "max":
                        cur[j] = max(cur[j], row[j])
                    elif a == "prod":
                        cur[j] *= row[j]
                    else:
                        cur[j] = a(cur[j], row[j])

    def result_frames(self, chunk: int):
        if not self.state:
            return
        items = list(self.state.items())
        nkey = self.schema.prefix
        for off in range(0, len(items), chunk):
            part = items[off:off + chunk]
            if nkey > 1:
                key_cols = list(zip(*[k for k, _ in part]))
            else:
                key_cols = [[k for k, _ in part]]
            val_cols = list(zip(*[v for _, v in part])) if part and \
                part[0][1] else []
            cols = [list(c) for c in key_cols] + [list(c) for c in val_cols]
            yield Frame.from_lists(cols, schema=self.schema)

    def num_keys(self) -> int:
        return len(self.state)
