"""Byte-order ranks of the rows of a BYTES column (K24): the order of
bytes.__lt__, by prefix refinement over 7-byte stretches
(csrc/bytes_order.hip).

Round w gives every still-undecided row one 64-bit key: its bytes
[7w, 7w+7) big-endian in the top 56 bits, zero-padded past the row's
end, and valid = clamp(len - 7w, 0, 7) in the low 8 bits.  As unsigned
integers two keys order as the two rows do on that stretch; equal keys
with valid < 7 mean equal rows, with valid == 7 the rows are still
tied.  A stable sort of the tied rows by (tie group, key) splits the
groups; the loop ends when no row is tied and unfinished, after at most
(longest common prefix of two tied rows) / 7 + 2 rounds, one small host
readback (the active count) per round.

A rank is the first position of the row's tie group in the final order:
it preserves order, is equal exactly for equal rows, and is not dense.

Every function takes a column (anything with .data, .offsets and
__len__, as frame.BytesColumn) of device or CPU tensors.  Device
tensors run the HIP kernels; CPU tensors run torch and give the same
result — the contract the device path is tested against.
"""

import torch

from .. import kernels as _k
from . import _C, native
from .sortedkeys import _uniq_starts, lex_argsort

# slots per workgroup of the refine kernel, rows per workgroup of the
# key kernel (csrc/bytes_order.hip)
REFINE_TILE_SLOTS = _C.BYTES_ORDER_TILE_SLOTS if _C is not None else 1024
KEYS_BLOCK = _C.BYTES_ORDER_BLOCK if _C is not None else 256


def round_keys(col, rows, w):
    """int64[m]: the round-w key of row rows[j] of `col`, top bit
    flipped so that the signed order of the result is the unsigned order
    of the keys.  A row index outside the column has length 0."""
    data, offsets = col.data, col.offsets
    w = int(w)
    if native(data.is_cuda, "bytes order keys"):
        return _k._C.bytes_order_keys(data.contiguous(),
                                      offsets.contiguous(), rows, w)
    n, m = offsets.shape[0] - 1, rows.shape[0]
    total = data.shape[0]
    ok = (rows >= 0) & (rows < n)
    r = torch.where(ok, rows, torch.zeros_like(rows))
    if n > 0:
        beg = torch.where(ok, offsets[r], torch.zeros_like(r))
        length = torch.where(ok, offsets[r + 1] - offsets[r],
                             torch.zeros_like(r))
    else:
        beg = length = torch.zeros_like(rows)
    valid = (length - 7 * w).clamp(0, 7)
    b = torch.arange(7, dtype=torch.int64, device=rows.device)
    idx = (beg + 7 * w).unsqueeze(1) + b
    real = (b < valid.unsqueeze(1)) & (idx >= 0) & (idx < total)
    if total:
        byts = data[idx.clamp(0, total - 1)].to(torch.int64)
    else:
        byts = torch.zeros((m, 7), dtype=torch.int64, device=rows.device)
    byts = torch.where(real, byts, torch.zeros_like(byts))
    # the top byte carries the flipped bit, as a signed byte: no overflow
    top = byts[:, 0] ^ 0x80
    key = (top - ((top & 0x80) << 1)) * (1 << 56) + valid
    for i in range(1, 7):
        key = key + (byts[:, i] << (56 - 8 * i))
    return key


def refine(grp_sorted, key_sorted):
    """(head int64[m], stay bool[m]) of slots sorted by (grp, key):
    head[j] = j where slot j differs from slot j-1 in grp or key (slot 0
    always), else 0; stay[j] where slot j is tied with a neighbour and
    its key's valid field is 7."""
    m = grp_sorted.shape[0]
    if native(grp_sorted.is_cuda, "bytes order refine"):
        head, stay = _k._C.bytes_order_refine(grp_sorted.contiguous(),
                                              key_sorted.contiguous())
        return head, stay
    dev = grp_sorted.device
    is_head = torch.ones(m, dtype=torch.bool, device=dev)
    is_head[1:] = ((grp_sorted[1:] != grp_sorted[:-1])
                   | (key_sorted[1:] != key_sorted[:-1]))
    next_head = torch.ones(m, dtype=torch.bool, device=dev)
    next_head[:-1] = is_head[1:]
    head = torch.where(is_head, torch.arange(m, device=dev),
                       torch.zeros(m, dtype=torch.int64, device=dev))
    stay = (~is_head | ~next_head) & ((key_sorted & 0xff) == 7)
    return head, stay


def distinct_order_ranks(col, stats=None):
    """int64[n] byte-order ranks of the rows of `col`.  Meant for
    distinct rows: it is correct for any rows, but a run of identical
    long rows stays tied to its last byte and sets the round count.
    stats, a dict, receives the number of rounds."""
    n = len(col)
    dev = col.offsets.device
    order = torch.arange(n, dtype=torch.int64, device=dev)
    grp = torch.zeros(n, dtype=torch.int64, device=dev)
    pos = order.clone() if n > 1 else order[:0]
    w = 0
    while pos.shape[0]:
        rows = order[pos]
        key = round_keys(col, rows, w)
        g = grp[pos]
        # (round 0: one group, the key alone sorts)
        o = lex_argsort([key] if w == 0 else [g, key])
        gs, ks = g[o], key[o]
        order[pos] = rows[o]
        head, stay = refine(gs, ks)
        grp[pos] = pos[torch.cummax(head, 0).values]
        pos = pos[stay]  # the round's one readback: the active count
        w += 1
    if stats is not None:
        stats["rounds"] = w
    rank = torch.empty_like(grp)
    rank[order] = grp
    return rank


def order_ranks(col, ids=None, stats=None):
    """int64[n] byte-order ranks of the rows of `col`, which may hold
    duplicates: rows are deduplicated by their 64-bit ids (col.ids64(),
    or `ids` when the caller has them), one exemplar per id is ranked,
    and the ranks go back to the rows.  Rows of equal id share a rank:
    exact up to the 2^-64-per-pair id collision BytesColumn accepts."""
    n = len(col)
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=col.offsets.device)
    if ids is None:
        ids = col.ids64()
    perm = lex_argsort([ids])
    _, starts = _uniq_starts([ids[perm]])
    if starts.shape[0] == n:
        return distinct_order_ranks(col, stats)
    ex_ranks = distinct_order_ranks(col.gather(perm[starts]), stats)
    run = torch.zeros(n, dtype=torch.int64, device=ids.device)
    run[starts] = 1
    rank = torch.empty_like(run)
    rank[perm] = ex_ranks[torch.cumsum(run, 0) - 1]
    return rank
