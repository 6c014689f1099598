"""Group-by aggregate over multi-column integer keys (K21): a streaming
device hash table keyed by a tuple of 2 to MAX_KEY_COLS int64 columns
(csrc/groupby_multi.hip).

Slots are claimed by a 64-bit fingerprint of the tuple, the tag; the
tuple itself is stored beside it and compared before anything is
accumulated.  Two tuples with one tag (2^-64 per pair at the default
width) raise the table's collision flag, and finish() then returns the
exact result of the caller's fallback over the retained batches.

fingerprint64 is the torch mirror of the device tag; it needs neither
the extension nor a device.  MultiKeyTable reads the BIGSLICE_GB_*
environment once, into an Options, when it is constructed.
"""

from __future__ import annotations

import dataclasses
import os
from typing import Callable, List, Optional, Sequence

import torch

from .. import kernels as _k
from . import _C, _require
from .groupby import (_AGG_CODES, _GB_VAL_DTYPES, GB_SENTINEL, MAX_PROBES,
                      HashTable)

# csrc/columns.h: most key columns, and most key + value columns (what
# groupby_compact takes)
MAX_KEY_COLS = _C.MAX_KEY_COLS if _C is not None else 8
MAX_COLS = _C.MAX_COLS if _C is not None else 16

_MK_KEY_DTYPES = (torch.int64, torch.int32)

# Seed of every combiner table (ext.hip GB_HASH_SEED).
GB_HASH_SEED = 0x9ACB0442

_MASK64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_FMIX_C1 = 0xFF51AFD7ED558CCD
_FMIX_C2 = 0xC4CEB9FE1A85EC53


@dataclasses.dataclass(frozen=True)
class Options:
    """The environment of the multi-column table, read once per table."""
    enabled: bool = True  # BIGSLICE_GB_MULTIKEY: 0 = lexicographic sort
    fp_bits: int = 64     # BIGSLICE_GB_FP_BITS: width of the tag

    @classmethod
    def from_env(cls, env=None) -> "Options":
        env = os.environ if env is None else env
        fp_bits = int(env.get("BIGSLICE_GB_FP_BITS", "64"))
        if not 1 <= fp_bits <= 64:
            raise ValueError("BIGSLICE_GB_FP_BITS must be in [1, 64]")
        return cls(enabled=env.get("BIGSLICE_GB_MULTIKEY", "1") != "0",
                   fp_bits=fp_bits)


def _i64(x: int) -> int:
    """The 64-bit word x as the int64 with the same bits."""
    x &= _MASK64
    return x - (1 << 64) if x >> 63 else x


def _lsr(h: torch.Tensor, s: int) -> torch.Tensor:
    """Logical shift right of int64 words (torch's >> is arithmetic)."""
    return (h >> s) & ((1 << (64 - s)) - 1)


def _fmix64(h: torch.Tensor) -> torch.Tensor:
    h = h ^ _lsr(h, 33)
    h = h * _i64(_FMIX_C1)  # int64 multiply wraps
    h = h ^ _lsr(h, 33)
    h = h * _i64(_FMIX_C2)
    return h ^ _lsr(h, 33)


def fingerprint64(cols: Sequence[torch.Tensor],
                  fp_bits: int = 64) -> torch.Tensor:
    """The tag of every row of the int64 key columns `cols`, as the
    device computes it: h = seed; per column, in order,
    h = fmix64((h + golden) ^ k); then h masked to fp_bits bits, and a
    tag equal to the empty marker becomes 0.  fmix64 is murmur3's 64-bit
    finalizer, a bijection; chaining it makes the tag depend on the
    order of the columns."""
    if not 1 <= fp_bits <= 64:
        raise ValueError("fp_bits must be in [1, 64]")
    h = torch.full_like(cols[0], GB_HASH_SEED, dtype=torch.int64)
    for c in cols:
        h = _fmix64((h + _i64(_GOLDEN)) ^ c.to(torch.int64))
    if fp_bits < 64:
        h = h & ((1 << fp_bits) - 1)
    return torch.where(h == GB_SENTINEL, torch.zeros_like(h), h)


def multikey_supported(key_dtypes, val_dtypes, aggs) -> bool:
    """Shapes MultiKeyTable takes: 2..MAX_KEY_COLS int64/int32 key
    columns, the plain insert's value dtypes and aggregations, and at
    most MAX_COLS columns in all."""
    key_dtypes, val_dtypes = list(key_dtypes), list(val_dtypes)
    return (2 <= len(key_dtypes) <= MAX_KEY_COLS
            and len(key_dtypes) + len(val_dtypes) <= MAX_COLS
            and all(dt in _MK_KEY_DTYPES for dt in key_dtypes)
            and all(dt in _GB_VAL_DTYPES for dt in val_dtypes)
            and all(isinstance(a, str) and a in _AGG_CODES for a in aggs))


class MultiKeyTable(HashTable):
    """Streaming device hash-aggregate keyed by a tuple of integer
    columns.  Follows GroupTable: batches are retained, a probe-chain
    overflow is noticed at finish() and answered by regrowing and
    re-inserting, and the host reads one {count, overflow, collision}
    triple per compaction and nothing per batch.

    fallback(key_cols, val_cols) -> (key_cols, val_cols) must group
    exactly; finish() calls it over the concatenated batches when two
    tuples shared a tag."""

    def __init__(self, nkey: int, val_dtypes, aggs: List[str], device,
                 cap_hint: Optional[int] = None,
                 fallback: Optional[Callable] = None):
        _require("multi-column groupby")
        self.opts = Options.from_env()
        self.nkey = nkey
        self.val_dtypes = list(val_dtypes)
        self.aggs = list(aggs)
        self.codes = [_AGG_CODES[a] for a in aggs]
        if not multikey_supported([torch.int64] * nkey, self.val_dtypes,
                                  self.aggs):
            raise ValueError("unsupported multi-column group-by shape")
        self.device = device
        self.cap_hint = cap_hint
        self.fallback = fallback
        self.key_dtypes: Optional[List[torch.dtype]] = None
        self.cap: Optional[int] = None
        self.tags = None   # [cap + 1] tuple fingerprints
        self.kcols: List = []  # [cap + 1] per key column
        self.tabs: List = []   # [cap + 1] aggregates per value column
        self.flags = None  # int32 {unused, overflow, collision}
        self.batches: List = []  # retained for re-insert and fallback
        self.rows = 0

    def _alloc(self, cap: int):
        self.cap = cap
        dev = self.device
        self.tags = torch.full((cap + 1,), GB_SENTINEL, dtype=torch.int64,
                               device=dev)
        self.kcols = [torch.empty(cap + 1, dtype=torch.int64, device=dev)
                      for _ in range(self.nkey)]
        self.tabs = self._agg_arrays(cap)
        self.flags = torch.zeros(3, dtype=torch.int32, device=dev)

    def _slots(self):
        return self.tags, self.kcols + self.tabs

    def insert(self, keys: List[torch.Tensor], vals: List[torch.Tensor]):
        if len(keys) != self.nkey or len(vals) != len(self.val_dtypes):
            raise ValueError("column count differs from the table's")
        dts = [k.dtype for k in keys]
        if self.key_dtypes is None:
            if not all(dt in _MK_KEY_DTYPES for dt in dts):
                raise TypeError("key columns must be int64 or int32")
            self.key_dtypes = dts
        elif dts != self.key_dtypes:
            raise TypeError("key dtypes differ from the first batch's")
        n = keys[0].shape[0]
        if n == 0:
            return
        self.rows += n
        # int32 key columns are widened here and narrowed at finish
        self._insert_now([k.to(torch.int64).contiguous() for k in keys],
                         [v.contiguous() for v in vals])

    def _insert_now(self, keys, vals):
        self._ensure_alloc(keys[0].shape[0])
        self.batches.append((keys, vals))
        _k._C.groupby_mk_insert(keys, vals, self.codes, self.tags, self.kcols,
                             self.tabs, self.flags, MAX_PROBES,
                             self.opts.fp_bits)

    def _narrow(self, keys):
        return [k if dt == torch.int64 else k.to(dt)
                for k, dt in zip(keys, self.key_dtypes)]

    def _drop(self):
        self.batches = []
        self.tags = self.flags = None
        self.kcols, self.tabs = [], []

    def finish(self):
        """Returns ([key columns], [vals]) of the aggregated groups."""
        from ..utils import stats
        stats.DEFAULT.add("combiner/records", self.rows)
        if self.cap is None:
            dts = self.key_dtypes or [torch.int64] * self.nkey
            return ([torch.empty(0, dtype=dt, device=self.device)
                     for dt in dts],
                    [torch.empty(0, dtype=dt, device=self.device)
                     for dt in self.val_dtypes])
        while True:
            outs, (ngroups, _, overflow, collision) = self._compact()
            if collision:
                # Two tuples share a tag: the table holds one of them and
                # skipped the other's rows.  Group the batches exactly.
                if self.fallback is None:
                    raise RuntimeError(
                        "multi-column group-by: fingerprint collision and "
                        "no fallback")
                stats.DEFAULT.add("combiner/fingerprint_fallbacks", 1)
                batches = self.batches
                kc = [torch.cat(cols) for cols in
                      zip(*(k for k, _ in batches))]
                vc = [torch.cat(cols) for cols in
                      zip(*(v for _, v in batches))]
                self._drop()
                keys, vals = self.fallback(kc, vc)
                keys, vals = list(keys), list(vals)
                break
            if overflow:
                self._regrow()
                continue
            keys = [o[:ngroups] for o in outs[1:1 + self.nkey]]
            vals = [o[:ngroups] for o in outs[1 + self.nkey:]]
            self.batches = []
            break
        stats.DEFAULT.add("combiner/keys", int(keys[0].shape[0]))
        return self._narrow(keys), vals
