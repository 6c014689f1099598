"""Group-by aggregate (K9): the streaming device hash table and the
rules that choose how batches are combined into it.

The rules are plain functions of numbers (choose_mode, part_plan,
regrow_capacity and the two fan-out rules): they need neither the
extension nor a device.  GroupTable reads the BIGSLICE_GB_* environment
once, into an Options, when it is constructed.
"""

from __future__ import annotations

import dataclasses
import math
import os
import sys
from typing import List, Optional

import torch

from .. import kernels as _k
from . import _C, native
from .sortedkeys import sort_combine

_AGG_CODES = {"sum": 0, "min": 1, "max": 2, "prod": 3}

_GB_KEY_DTYPES = (torch.int64,)
_GB_VAL_DTYPES = (torch.int64, torch.int32, torch.float32, torch.float64)

GB_SENTINEL = -(1 << 63)
MAX_PROBES = 128

# Geometry of the partitioned insert (csrc/groupby_part.hip): pairs per
# aggregate tile, slots of its LDS table, largest bucket fan-out.
PART_TILE_ROWS = _C.GBP_TILE_ROWS if _C is not None else None
PART_LDS_SLOTS = _C.GBP_LDS_SLOTS if _C is not None else None
PART_MAX_BUCKETS = _C.GBP_MAX_BUCKETS if _C is not None else None

# Rows an owner workgroup of the bucket-owning aggregate takes from its
# segment; the rest of an oversize bucket goes to the tiled cleanup pass.
PART_OWN_LIMIT = _C.GBP_OWN_LIMIT if _C is not None else None


@dataclasses.dataclass(frozen=True)
class Options:
    """The BIGSLICE_GB_* environment, read once per GroupTable."""
    mode: Optional[str] = None  # BIGSLICE_GB_MODE: lds | global | part
    combine: str = "auto"       # BIGSLICE_GB_COMBINE: auto | hash | sort
    part: bool = True           # BIGSLICE_GB_PART: "part" in the chooser
    part_owned: bool = True     # BIGSLICE_GB_PART_OWNED: owned slices
    part_group: int = 0         # BIGSLICE_GB_PART_GROUP: scatter tiles per
                                # workgroup, 0 = the extension's rule
    lds_blocks: int = 4096      # BIGSLICE_GB_LDS_BLOCKS: grid cap, "lds"
    sample_rows: int = 1 << 19  # BIGSLICE_GB_SAMPLE_ROWS
    sample: str = "hash"        # BIGSLICE_GB_SAMPLE: hash | sort (the
                                # distinct count of the sampled prefix)
    finish_part: bool = True    # BIGSLICE_GB_FINISH_PART: the table
                                # finishes straight into partitions
    debug: bool = False         # BIGSLICE_GB_DEBUG: chooser trace

    @classmethod
    def from_env(cls, env=None) -> "Options":
        env = os.environ if env is None else env
        mode = env.get("BIGSLICE_GB_MODE")
        return cls(
            mode=mode if mode in ("lds", "global", "part") else None,
            combine=env.get("BIGSLICE_GB_COMBINE", "auto"),
            part=env.get("BIGSLICE_GB_PART", "1") == "1",
            part_owned=env.get("BIGSLICE_GB_PART_OWNED", "1") == "1",
            part_group=int(env.get("BIGSLICE_GB_PART_GROUP", "0")),
            lds_blocks=int(env.get("BIGSLICE_GB_LDS_BLOCKS", "4096")),
            sample_rows=int(env.get("BIGSLICE_GB_SAMPLE_ROWS",
                                    str(1 << 19))),
            sample=("sort" if env.get("BIGSLICE_GB_SAMPLE") == "sort"
                    else "hash"),
            finish_part=env.get("BIGSLICE_GB_FINISH_PART", "1") == "1",
            debug=bool(env.get("BIGSLICE_GB_DEBUG")))


def _next_pow2(n: int, floor: int = 1024) -> int:
    c = floor
    while c < n:
        c <<= 1
    return c


def first_capacity(cap_hint: Optional[int], n: int, floor: int = 1024) -> int:
    """Capacity of a table whose first batch has n rows: the caller's
    hint, else two slots per row up to config.GROUPBY_INITIAL_CAP."""
    from .. import config
    return _next_pow2(cap_hint or min(
        2 * n, getattr(config, "GROUPBY_INITIAL_CAP", 1 << 23)), floor)


def part_buckets(n: int, nkeys: float, cap: int,
                 lds_slots: int = PART_LDS_SLOTS,
                 tile_rows: int = PART_TILE_ROWS,
                 max_buckets: int = PART_MAX_BUCKETS) -> int:
    """Bucket fan-out B (a power of two) of the partitioned insert for a
    batch of n rows over ~nkeys keys.  A tile of T pairs spans at most
    T/(n/B) + 1 buckets of nkeys/B keys each; B is the smallest fan-out
    that keeps that count within half the LDS table:
    T*nkeys/n + nkeys/B <= slots/2.  Clamped to [2, max_buckets] and to
    the table capacity (bucket id = high bits of the slot)."""
    room = lds_slots / 2 - tile_rows * nkeys / max(n, 1)
    b = 2
    while b < max_buckets and (room <= 0 or b * room < nkeys):
        b <<= 1
    return min(b, cap)


def part_owned_buckets(n: int, cap: int, lds_slots: int, tile_rows: int,
                       max_buckets: int):
    """(B, S) of the bucket-owning aggregate pass for n rows into a table
    of cap slots, or None when it does not apply.  A workgroup owns the
    table slice of one bucket, S = cap / B slots, in LDS, so S must not
    exceed lds_slots; and there should be about as many workgroups as
    the tiled pass has tiles, to fill the chip.  B is the smallest power
    of two >= max(cap / lds_slots, n / tile_rows), clamped to
    [2, min(max_buckets, cap)]."""
    want = max(cap / lds_slots, n / tile_rows)
    b = 2
    while b < want:
        b <<= 1
    b = max(2, min(b, max_buckets, cap))
    s = cap // b
    return (b, s) if s <= lds_slots else None


# "part" (partitioned LDS pre-aggregation, K19) pays three extra
# streaming passes to turn ~rows/key global atomics per key per batch
# into one per key per tile; below a few rows per key per batch there
# is nothing to absorb.
PART_BAND = (6.0, 500.0)  # rows per key per batch


def forced_mode(opts: Options, sum_i64: bool) -> Optional[str]:
    """The combine mode the options fix without a cardinality sample, or
    None.  (A forced "part" still samples: it sizes the table and the
    bucket fan-out from the key estimate exactly as the chooser would.)"""
    if opts.mode in ("lds", "global"):
        return opts.mode
    if opts.mode == "part" and not sum_i64:
        return "global"  # single int64 sum only
    if opts.combine == "sort":
        return "sort"
    return None


def choose_mode(distinct: int, sample_n: int, batch_n: int, sum_i64: bool,
                opts: Options, cap_hint: Optional[int] = None):
    """Combine strategy from a sample of sample_n rows of a batch_n-row
    batch that held `distinct` keys.  Returns (mode, key_estimate,
    cap_hint): key_estimate is None when the sample saturated, and a
    caller-given cap_hint comes back unchanged.  Three regimes (measured
    at 125M rows, profiles/sortcombine_crossover_r2.txt):
    * few keys (d <= s/32 ~ 16k): LDS-tier hash, 2.7 ms at 1k;
    * contended hash (rows/key >~ 500): the memory-side atomic
      unit serializes same-slot adds — insert 10.3 ms vs
      sort+segment-reduce 3.9 ms at 64k keys x 1900 rows/key;
    * wide keys (sample ~saturated, K >~ 2M): sort; a right-sized
      insert is 6.2 ms at 10M keys but the sort path stays ~5.1.
    In between (e.g. the north-star consumer shape, ~125 rows/key)
    the streaming insert wins IN CONTEXT (it overlaps with reads;
    the sort path bunches all work at finish): stay on the
    streaming insert — "part" (partitioned LDS pre-aggregation)
    for the int64-sum shape inside PART_BAND, else "global".
    BIGSLICE_GB_MODE=part overrides the verdict;
    BIGSLICE_GB_COMBINE=hash turns a "sort" verdict into "global"."""
    forced = forced_mode(opts, sum_i64)
    if forced:
        return forced, None, cap_hint
    s = sample_n
    K = None
    # Invert d = K(1-e^(-s/K)) to estimate the key-space size and
    # presize the table: the 10M-key hash insert measured 6.2 ms
    # properly sized vs 22 ms through the overflow-regrow grind.
    if distinct < s:
        K = float(distinct)
        for _ in range(20):
            K = distinct / (1.0 - math.exp(-s / K))
        if cap_hint is None:
            cap_hint = _next_pow2(min(max(int(4 * K), 1024), 1 << 30))
    if distinct * 32 <= s:
        mode = "lds"
    elif distinct * 100 > s * 88:
        mode = "sort"  # sample ~saturated: K at least ~2M
    else:
        rows_per_key = batch_n / max(K, 1.0)
        mode = "sort" if rows_per_key > 500 else "global"
        if (mode == "global" and sum_i64 and opts.part
                and PART_BAND[0] <= rows_per_key <= PART_BAND[1]):
            mode = "part"
    if opts.mode == "part":
        mode = "part"
    elif mode == "sort" and opts.combine == "hash":
        mode = "global"
    return mode, K, cap_hint


def part_plan(n: int, cap: int, key_estimate: Optional[float],
              opts: Options, lds_slots: int, tile_rows: int,
              max_buckets: int, min_rows: int):
    """How a "part" table inserts one batch of n rows: ("owned", B),
    ("tiled", B), or None for the plain insert (under min_rows the
    passes' fixed cost dominates; the kernels index rows with 31 bits)."""
    if not min_rows <= n < (1 << 31):
        return None
    own = part_owned_buckets(n, cap, lds_slots, tile_rows,
                             max_buckets) if opts.part_owned else None
    if own is not None:
        return "owned", own[0]
    nkeys = key_estimate or cap / 4
    return "tiled", part_buckets(n, nkeys, cap, lds_slots, tile_rows,
                                 max_buckets)


def regrow_capacity(cap: int, rows: int) -> int:
    """Capacity after a probe-chain overflow at cap slots with `rows`
    rows inserted so far: 4 slots per row (rows bound the keys), at
    least a doubling."""
    new = cap
    while new < 4 * rows and new < (1 << 30):
        new <<= 1
    if new == cap:
        new <<= 1
    if new > (1 << 31):
        raise RuntimeError("groupby table overflow")
    return new


def groupby_supported(keys: torch.Tensor, vals: List[torch.Tensor],
                      aggs: List[str]) -> bool:
    return (native(keys.is_cuda, "groupby") and groupby_shape_supported(
        [keys.dtype], [v.dtype for v in vals], aggs))


def groupby_shape_supported(key_dtypes, val_dtypes, aggs) -> bool:
    """Shapes GroupTable takes: one int64 key column, the plain insert's
    value dtypes and aggregations."""
    return (all(dt in _GB_KEY_DTYPES for dt in key_dtypes)
            and all(dt in _GB_VAL_DTYPES for dt in val_dtypes)
            and all(isinstance(a, str) and a in _AGG_CODES for a in aggs))


class HashTable:
    """The lifecycle GroupTable and MultiKeyTable share: capacity from
    the first batch, batches retained, one readback per compaction, and
    a probe-chain overflow answered by a larger table and a re-insert.
    A subclass has _alloc(cap), _insert_now(keys, vals), _slots() and the
    attributes device, val_dtypes, codes, cap, cap_hint, flags, batches
    and rows."""

    def _ensure_alloc(self, n: int):
        if self.cap is None:
            self._alloc(first_capacity(self.cap_hint, n))

    def _agg_arrays(self, cap: int) -> List:
        """[cap + 1] aggregates per value column, at the identity."""
        return [
            _k._C.agg_identity(torch.empty(0, dtype=dt, device=self.device),
                            code, cap + 1)
            for dt, code in zip(self.val_dtypes, self.codes)]

    def _compact(self):
        """One compaction and its one readback: (outs, [count, *flags])."""
        cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
        outs = _k._C.groupby_compact(*self._slots(), cursor)
        host = torch.cat([cursor, self.flags.to(torch.int64)]).cpu()
        return outs, host.tolist()

    def _regrow(self):
        batches = self.batches
        self._alloc(regrow_capacity(self.cap, self.rows))
        self.batches = []
        for keys, vals in batches:
            self._insert_now(keys, vals)


class GroupTable(HashTable):
    """Streaming device hash-aggregate (K9): an open-addressing table in
    HBM that multiple batches insert into; finish() compacts used slots.
    On probe-chain overflow the table doubles and re-inserts all retained
    batches (the reference combiner's grow-x2, exec/combiner.go:47)."""

    # A batch of at least _SMALL_BATCH rows triggers the cardinality
    # sample; smaller ones (e.g. pre-combined shuffle buckets on the
    # consumer side) wait for it, or for finish.
    _SMALL_BATCH = 1 << 21
    # Batches of a "part" table under _PART_MIN_ROWS take the plain
    # insert.
    _PART_MIN_ROWS = 1 << 21

    def __init__(self, val_dtypes, aggs: List[str], device,
                 cap_hint: int = None):
        self.opts = Options.from_env()
        self.aggs = aggs
        self.codes = [_AGG_CODES[a] for a in aggs]
        self.device = device
        self.val_dtypes = list(val_dtypes)
        self.cap = None
        self.cap_hint = cap_hint
        self.tkeys = None  # [cap + 1] keys; slot cap holds the sentinel key
        self.tabs: List = []  # [cap + 1] aggregates, one per value column
        self.flags = None  # int32 {sentinel_seen, overflow}
        self.batches: List = []  # retained for overflow re-insert
        self._deferred: List = []  # awaiting the combine-mode decision
        self.rows = 0
        # None (undecided), "pending" (sample in flight), or the decision:
        # "lds", "global", "part", "sort"
        self._mode: Optional[str] = None
        self._sample_forced: Optional[str] = None
        self._sample_n = 0
        self._sample_batch_n = 0
        self._sample_ne = None  # device scalar: key changes in the sample
        self._key_estimate: Optional[float] = None
        self._settled = False  # _settle has run
        self._done = None  # its result, when that is not in the table

    @property
    def _sum_i64(self) -> bool:
        return (len(self.val_dtypes) == 1
                and self.val_dtypes[0] == torch.int64
                and self.aggs == ["sum"])

    def _alloc(self, cap: int):
        self.cap = cap
        dev = self.device
        self.tkeys = torch.full((cap + 1,), GB_SENTINEL,
                                dtype=torch.int64, device=dev)
        self.tabs = self._agg_arrays(cap)
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)

    def _slots(self):
        return self.tkeys, self.tabs

    @property
    def _sort_combinable(self) -> bool:
        """Shapes sortedkeys.sort_combine handles: sum/min/max over
        numeric columns (its float sums are run-to-run reproducible —
        unlike the hash table's atomic adds).  These shapes defer their
        batches until a sampled cardinality has chosen the combine mode."""
        return (_k._C is not None
                and str(self.device).startswith("cuda")
                and all(a in ("sum", "min", "max") for a in self.aggs)
                and all(dt in _GB_VAL_DTYPES for dt in self.val_dtypes))

    def _start_sample(self, keys: torch.Tensor) -> None:
        """Cardinality sample: the exact count of distinct keys in a
        prefix of the first large batch, minus one, as a device scalar.
        Launched WITHOUT a host sync (the scalar is read at the next
        insert or at finish).  "hash" claims the keys in a scratch tag
        table (csrc/groupby.hip, two launches); "sort" sorts the prefix
        and counts the key changes (24 launches at 2^19 rows): the same
        number either way."""
        self._sample_forced = forced_mode(self.opts, self._sum_i64)
        if self._sample_forced:
            return
        prefix = min(keys.shape[0], self.opts.sample_rows)
        self._sample_n = prefix
        self._sample_batch_n = keys.shape[0]
        if self.opts.sample == "hash" and native(keys.is_cuda, "groupby"):
            self._sample_ne = _k._C.groupby_sample_distinct(
                keys.contiguous(), prefix)
            return
        # probe=False: the probe's count readback would sync the
        # stream; the sample must stay fire-and-forget
        sk = _k._C.radix_sort_keys(keys[:prefix].contiguous(),
                                probe=False)
        self._sample_ne = (sk[1:] != sk[:-1]).sum()  # device scalar

    def _read_sample(self) -> str:
        """The combine mode, from the options or the sample (one sync)."""
        if self._sample_forced:
            return self._sample_forced
        distinct = 1 + int(self._sample_ne.item())
        mode, self._key_estimate, self.cap_hint = choose_mode(
            distinct, self._sample_n, self._sample_batch_n, self._sum_i64,
            self.opts, self.cap_hint)
        if self.opts.debug:
            print(f"[gb] sample={self._sample_n} distinct={distinct} "
                  f"cap_hint={self.cap_hint} mode={mode}",
                  file=sys.stderr, flush=True)
        return mode

    def insert(self, keys: torch.Tensor, vals: List[torch.Tensor]):
        n = keys.shape[0]
        if n == 0:
            return
        self.rows += n
        if not self._sort_combinable:
            self._insert_now(keys, vals)
            return
        if self._mode is None:
            if n >= self._SMALL_BATCH:
                # First large batch: kick the async cardinality sample
                # and defer; the decision is read at the NEXT insert
                # (or at finish), when the 512k-row sample compute is
                # long finished — the streaming path never stalls on
                # it.  (Provisionally hash-inserting this batch while
                # the sample flies was MEASURED: no gain at 1M keys —
                # the probe-free sample already streams — and 2x worse
                # at 10M keys, where the un-presized provisional table
                # hits the overflow-regrow grind.  Deferral stays.)
                self._start_sample(keys)
                self._mode = "pending"
            self._deferred.append((keys, vals))
            return
        if self._mode == "pending":
            self._mode = self._read_sample()
        if self._mode == "sort":
            self._deferred.append((keys, vals))
            return
        self._flush_deferred()  # pre-decision batches
        self._insert_now(keys, vals)

    def _flush_deferred(self):
        pending, self._deferred = self._deferred, []
        for k, v in pending:
            self._insert_now(k, v)

    def _insert_now(self, keys: torch.Tensor, vals: List[torch.Tensor]):
        """Allocate on demand and run the insert kernel of the decided
        mode.  Only "lds" and "part" have kernels of their own (both for
        the single int64 sum); every other state of _mode, undecided and
        "sort" (its merge into a provisional table) included, takes the
        plain one-pass insert."""
        self._ensure_alloc(keys.shape[0])
        self.batches.append((keys, vals))
        mode = self._mode if self._sum_i64 else None
        plan = part_plan(
            keys.shape[0], self.cap, self._key_estimate, self.opts,
            PART_LDS_SLOTS, PART_TILE_ROWS, PART_MAX_BUCKETS,
            self._PART_MIN_ROWS) if mode == "part" else None
        if mode == "lds":
            _k._C.groupby_insert_lds(keys, vals[0], self.tkeys, self.tabs[0],
                                  self.flags, MAX_PROBES,
                                  self.opts.lds_blocks)
        elif plan is not None:
            kind, nbuckets = plan
            _k._C.groupby_insert_part(keys, vals[0], self.tkeys, self.tabs[0],
                                   self.flags, MAX_PROBES, nbuckets,
                                   1 if kind == "owned" else 0,
                                   self.opts.part_group)
        else:
            _k._C.groupby_insert(keys, list(vals), self.codes, self.tkeys,
                              self.tabs, self.flags, MAX_PROBES)

    def _finish_deferred(self):
        """Combine the deferred batches at finish.  Mode "sort":
        sort+segment-reduce them; when a provisional table exists, the
        combined uniques merge into it and compaction follows.  Mode
        None (all batches were small): decide from a sample now.
        Returns (keys, vals), or None when the result is in the table."""
        from ..utils import stats
        if self._mode not in (None, "sort"):
            self._flush_deferred()
            return None
        batches = self._deferred
        keys = (batches[0][0] if len(batches) == 1
                else torch.cat([k for k, _ in batches]))
        if self._mode is None:
            self._start_sample(keys)
            self._mode = self._read_sample()
            if self._mode != "sort":
                self._flush_deferred()
                return None
        self._deferred = []
        vcols = (list(batches[0][1]) if len(batches) == 1
                 else [torch.cat(cols)
                       for cols in zip(*(v for _, v in batches))])
        uk, outs = sort_combine(keys, vcols, self.codes)
        if self.cap is not None:
            # merge with the provisionally hash-inserted batches
            self._insert_now(uk, outs)
            return None
        stats.DEFAULT.add("combiner/keys", int(uk.shape[0]))
        return uk, outs

    def _settle(self):
        """What finish does before it reads the table, once: the pending
        sample, the deferred batches.  Returns (keys, [vals]) when the
        result is not in a table (sort mode without a provisional table,
        no rows), else None."""
        from ..utils import stats
        if self._settled:
            return self._done
        self._settled = True
        stats.DEFAULT.add("combiner/records", self.rows)
        if self._mode == "pending":
            self._mode = self._read_sample()
        if self._deferred:
            self._done = self._finish_deferred()
        if self._done is None and self.cap is None:
            empty = torch.empty(0, dtype=torch.int64, device=self.device)
            self._done = empty, [
                torch.empty(0, dtype=dt, device=self.device)
                for dt in self.val_dtypes]
        return self._done

    def finish_partitioned(self, nparts: int):
        """finish() for a shuffle producer: the aggregated groups split
        into nparts hash partitions (hash_row over the key, seed 0,
        % nparts: what hash_partition gives), as a list of (keys, [vals])
        slices of one buffer, by one pass over the table and one
        readback (csrc/groupby_finish.hip).  None where that does not
        apply (BIGSLICE_GB_FINISH_PART=0, a fan-out the kernels do not
        take, a result that is not in a table): finish() then gives the
        result, as ever."""
        from ..utils import stats
        if not (self.opts.finish_part
                and 1 <= nparts <= _k._C.MAX_LDS_PARTS):
            return None
        if self._settle() is not None:
            return None
        while True:
            outs, host = _k._C.groupby_compact_partition(
                self.tkeys, self.tabs, self.flags, nparts)
            *counts, _, overflow = host.tolist()
            if overflow:
                self._regrow()
                continue
            self.batches = []
            stats.DEFAULT.add("combiner/keys", sum(counts))
            parts, off = [], 0
            for c in counts:
                parts.append((outs[0][off:off + c],
                              [o[off:off + c] for o in outs[1:]]))
                off += c
            return parts

    def finish(self):
        """Returns (keys, [vals]) of the aggregated groups."""
        from ..utils import stats
        done = self._settle()
        if done is not None:
            return done
        while True:
            outs, (nkeys, sentinel_seen, overflow) = self._compact()
            if overflow:
                self._regrow()
                continue
            keys = outs[0][:nkeys]
            vals = [o[:nkeys] for o in outs[1:]]
            if sentinel_seen:
                keys = torch.cat([keys, torch.full(
                    (1,), GB_SENTINEL, dtype=torch.int64,
                    device=self.device)])
                vals = [torch.cat([v, t[self.cap:self.cap + 1]])
                        for v, t in zip(vals, self.tabs)]
            self.batches = []
            stats.DEFAULT.add("combiner/keys", int(keys.shape[0]))
            return keys, vals


def groupby(keys: torch.Tensor, vals: List[torch.Tensor],
            aggs: List[str]):
    """One-shot hash-aggregate: returns (unique_keys, [combined vals])."""
    t = GroupTable([v.dtype for v in vals], aggs, keys.device)
    t.insert(keys, list(vals))
    return t.finish()
