"""Id dictionary (K23): a device hash table from the 64-bit id of a
string (BytesColumn.ids64) to the position of one exemplar row in an
append-only dictionary of strings (csrc/iddict.hip), and the
variable-length row gather that collects the exemplars
(csrc/bytes_gather.hip).

Contract: every id of every added row resolves, through lookup(), to a
position of strings() whose bytes equal that row's bytes (up to the
2^-64-per-pair id collision BytesColumn accepts).  An id equal to the
empty marker is treated as id 0.  The order of the dictionary is not
part of the contract: on the device it depends on atomic arrival order.

Device tensors run the HIP kernels; CPU tensors run a host mirror with
the same contract.
"""

from __future__ import annotations

from typing import List, Optional

import torch

from .. import kernels as _k
from . import _C, _require
from .groupby import GB_SENTINEL, MAX_PROBES, _next_pow2, first_capacity

_MAX_CAP = 1 << 30  # capacity is a power of two below 2^31


_CAP_FLOOR = 16  # the smallest table


def bytes_gather(data: torch.Tensor, offsets: torch.Tensor,
                 rows: torch.Tensor, total: Optional[int] = None):
    """Rows `rows` of the device BYTES column (data, offsets) as
    (out_data, out_offsets), zero-based.  offsets may be a slice.  total
    is the byte count of the result when the caller knows it; None reads
    it back (one host readback)."""
    _require("bytes_gather")
    out = _k._C.bytes_gather(data.contiguous(), offsets.contiguous(), rows,
                          -1 if total is None else int(total))
    return out[0], out[1]


class IdDictionary:
    """Streaming dictionary id -> exemplar string."""

    def __init__(self, device, cap_hint: Optional[int] = None):
        self.device = torch.device(device)
        self.on_device = self.device.type == "cuda"
        if self.on_device:
            _require("id dictionary")
        self.cap_hint = cap_hint
        self.cap: Optional[int] = None
        self.tags = None   # int64[cap + 1] ids, GB_SENTINEL = empty
        self.ref = None    # int64[cap + 1] positions
        self.regrows = 0
        self._n = 0        # strings in the dictionary
        self._nbytes = 0
        self._chunks: List = []  # BytesColumn exemplars, position order
        self._chunk_bytes: List[int] = []
        self._strings = None
        self._host = {}    # the CPU mirror's table

    def __len__(self) -> int:
        return self._n

    # -- device table ------------------------------------------------------

    def _probes(self, cap: int) -> int:
        return min(MAX_PROBES, cap)

    def _alloc(self, cap: int):
        if cap > _MAX_CAP:
            raise RuntimeError("id dictionary overflow")
        tags = torch.full((cap + 1,), GB_SENTINEL, dtype=torch.int64,
                          device=self.device)
        ref = torch.empty(cap + 1, dtype=torch.int64, device=self.device)
        return tags, ref

    def _regrow(self, cap: int):
        """Move the table into one of at least `cap` slots."""
        self.regrows += 1
        while True:
            tags, ref = self._alloc(cap)
            flag = torch.zeros(1, dtype=torch.int32, device=self.device)
            _k._C.iddict_rehash(self.tags, self.ref, tags, ref, flag,
                             self._probes(cap))
            if not int(flag.item()):  # only on the regrow path
                break
            cap <<= 1
        self.cap, self.tags, self.ref = cap, tags, ref

    def _append(self, chunk, nbytes: int):
        self._chunks.append(chunk)
        self._chunk_bytes.append(nbytes)
        self._n += len(chunk)
        self._nbytes += nbytes
        self._strings = None

    def add(self, ids: torch.Tensor, col) -> None:
        """Add the rows of the BYTES column `col`, whose ids are `ids`."""
        n = ids.shape[0]
        if n != len(col):
            raise ValueError("one id per row")
        if n == 0:
            return
        if not self.on_device:
            return self._add_host(ids, col)
        ids = ids.contiguous()
        if self.cap is None:
            self.cap = first_capacity(self.cap_hint, n, _CAP_FLOOR)
            self.tags, self.ref = self._alloc(self.cap)
        lens = col.lengths().contiguous()
        while True:
            counters = torch.zeros(3, dtype=torch.int64, device=self.device)
            newrows = _k._C.iddict_claim(ids, lens, self.tags, self.ref,
                                      self._n, counters,
                                      self._probes(self.cap))
            # the one host readback per run of the claim
            m, nbytes, overflow = counters.tolist()
            if m:
                data, offs = bytes_gather(col.data, col.offsets,
                                          newrows[:m], nbytes)
                from ..frame import BytesColumn
                self._append(BytesColumn(data, offs), nbytes)
            if not overflow:
                break
            # Rows were left out.  Regrow and run the claim over the same
            # batch again: the rows of this run are found, the rest are
            # appended after them.
            self._regrow(max(2 * self.cap,
                             _next_pow2(4 * self._n, _CAP_FLOOR)))
        if 2 * self._n > self.cap:
            self._regrow(_next_pow2(4 * self._n, _CAP_FLOOR))

    def lookup(self, ids: torch.Tensor) -> torch.Tensor:
        """The position of every id, -1 when absent."""
        if not self.on_device:
            return self._lookup_host(ids)
        ids = ids.to(self.device).contiguous()
        if self.cap is None:
            return torch.full_like(ids, -1)
        return _k._C.iddict_lookup(ids, self.tags, self.ref,
                                self._probes(self.cap))

    def strings(self):
        """The dictionary as one BytesColumn, in position order."""
        from ..frame import BytesColumn
        if self._strings is None:
            if not self._chunks:
                self._strings = BytesColumn(
                    torch.empty(0, dtype=torch.uint8, device=self.device),
                    torch.zeros(1, dtype=torch.int64, device=self.device))
            elif len(self._chunks) == 1:
                self._strings = self._chunks[0]
            else:
                # the chunks are zero-based and their byte counts known on
                # the host: one concatenation, no readback
                offs, off = [], 0
                for c, nb in zip(self._chunks, self._chunk_bytes):
                    offs.append(c.offsets[:-1] + off)
                    off += nb
                offs.append(torch.tensor([off], dtype=torch.int64,
                                         device=self.device))
                self._strings = BytesColumn(
                    torch.cat([c.data for c in self._chunks]),
                    torch.cat(offs))
                self._chunks = [self._strings]
                self._chunk_bytes = [off]
        return self._strings

    # -- host mirror -------------------------------------------------------

    @staticmethod
    def _norm(i: int) -> int:
        return 0 if i == GB_SENTINEL else i

    def _add_host(self, ids: torch.Tensor, col) -> None:
        table = self._host
        new = []
        for row, i in enumerate(ids.tolist()):
            i = self._norm(i)
            if i not in table:
                table[i] = self._n + len(new)
                new.append(row)
        if new:
            chunk = col.select(torch.tensor(new, dtype=torch.int64))
            self._append(chunk, int(chunk.data.shape[0]))

    def _lookup_host(self, ids: torch.Tensor) -> torch.Tensor:
        table = self._host
        return torch.tensor([table.get(self._norm(i), -1)
                             for i in ids.tolist()], dtype=torch.int64)
