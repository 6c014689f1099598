"""Operations on key-sorted arrays: run boundaries (K18), the
sorted-unique merge, their multi-column forms with a lexicographic
sort and search (K22), and the sort-combine pipeline (K6 sort + K16
segmented reduction).

Every function takes and returns torch tensors.  A device tensor goes to
the HIP extension; a CPU tensor runs a torch implementation that gives
the same result — the contract the device path is tested against.
"""

import torch

from . import _C, ALLOW_FALLBACK, _require

SEGREDUCE_MAX_RUN = 4096  # longest run k_segreduce takes, a thread per run
_SCATTER_OP = ("sum", "amin", "amax")  # by aggregation code


def _native(t, feature):
    """Whether t goes to the extension; a device tensor needs one."""
    if _C is None:
        if t.is_cuda and not ALLOW_FALLBACK:
            _require(feature)
        return False
    return t.is_cuda


def _uniq_starts(sorted_keys):
    """(unique_keys, run_starts) of a SORTED array, one readback.
    Device int64: ONE pass (_C.runs_sorted, 8 B/row read); otherwise
    diff mask + nonzero + gather (3 reads of the key array + a bool-mask
    round trip)."""
    n = sorted_keys.shape[0]
    if n and sorted_keys.dtype == torch.int64 and _native(sorted_keys, "runs"):
        uniq, starts, cnt = _C.runs_sorted(sorted_keys.contiguous())
        c = int(cnt.item())
        return uniq[:c], starts[:c]
    mask = torch.ones(n, dtype=torch.bool, device=sorted_keys.device)
    mask[1:] = sorted_keys[1:] != sorted_keys[:-1]
    starts = mask.nonzero(as_tuple=True)[0]
    return sorted_keys[starts], starts


def runs(sorted_keys):
    """(unique_keys, starts, ends) of the runs of a SORTED key array."""
    n, dev = sorted_keys.shape[0], sorted_keys.device
    if n == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return e, e, e
    uniq, starts = _uniq_starts(sorted_keys)
    ends = torch.cat([starts[1:],
                      torch.tensor([n], dtype=torch.int64, device=dev)])
    return uniq, starts, ends


def unique_sorted(sorted_keys):
    """The distinct keys of a SORTED array, in order."""
    return _uniq_starts(sorted_keys)[0]


def merge_sorted_unique(a, b):
    """Sorted-unique union of two SORTED key arrays via searchsorted
    scatter (2 passes; ~3x cheaper than re-sorting the concatenation)."""
    n, m = a.shape[0], b.shape[0]
    pos_a = (torch.arange(n, device=a.device)
             + torch.searchsorted(b, a, right=False))
    pos_b = (torch.arange(m, device=a.device)
             + torch.searchsorted(a, b, right=True))
    merged = torch.empty(n + m, dtype=a.dtype, device=a.device)
    merged[pos_a] = a
    merged[pos_b] = b
    return unique_sorted(merged)


# -- multi-column keys (K22) ------------------------------------------------
#
# A key is a tuple of integer columns, first column most significant.
# The extension takes contiguous int64 columns: int32 columns are widened
# on the way in and narrowed on the way out, as MultiKeyTable does.

# rows per tile of the run-boundary kernels (csrc/runs_multi.hip)
MRUNS_TILE_ROWS = _C.MRUNS_TILE_ROWS if _C is not None else 4096


def _wide(cols):
    return [c.to(torch.int64).contiguous() for c in cols]


def lex_argsort(cols):
    """Stable permutation sorting the rows of `cols` lexicographically:
    one stable sort per column from the last to the first (device: the
    radix argsort, stable on both of its engines; CPU: torch.sort)."""
    cols = list(cols)
    native = _native(cols[0], "lex_argsort")
    perm = None
    for c in reversed(cols):
        k = c if perm is None else c[perm]
        if native:
            o = _C.radix_argsort(k.contiguous())
        else:
            o = torch.sort(k, stable=True).indices
        perm = o if perm is None else perm[o]
    return perm


def _uniq_starts_multi(sorted_cols):
    """([distinct tuples per column], run_starts) of lexicographically
    SORTED columns of n > 0 rows, one readback."""
    n = sorted_cols[0].shape[0]
    if _native(sorted_cols[0], "runs_multi"):
        uniq, starts, cnt = _C.runs_multi(_wide(sorted_cols))
        c = int(cnt.item())
        return ([u[:c] if s.dtype == torch.int64 else u[:c].to(s.dtype)
                 for u, s in zip(uniq, sorted_cols)], starts[:c])
    mask = torch.zeros(n, dtype=torch.bool, device=sorted_cols[0].device)
    mask[0] = True
    for c in sorted_cols:
        mask[1:] |= c[1:] != c[:-1]
    starts = mask.nonzero(as_tuple=True)[0]
    return [c[starts] for c in sorted_cols], starts


def runs_multi(sorted_cols):
    """(unique tuple columns, starts, ends) of the runs of
    lexicographically SORTED key columns."""
    sorted_cols = list(sorted_cols)
    n, dev = sorted_cols[0].shape[0], sorted_cols[0].device
    if n == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return [c[:0] for c in sorted_cols], e, e
    uniq, starts = _uniq_starts_multi(sorted_cols)
    ends = torch.cat([starts[1:],
                      torch.tensor([n], dtype=torch.int64, device=dev)])
    return uniq, starts, ends


def unique_sorted_multi(sorted_cols):
    """The distinct tuples of lexicographically SORTED columns, in order,
    one tensor per column."""
    return runs_multi(sorted_cols)[0]


def lex_searchsorted(sorted_cols, query_cols, right=False):
    """torch.searchsorted over tuples: for every query tuple, the first
    position among the lexicographically SORTED tuples whose tuple is
    >= the query (right=False) or > the query (right=True).  int64[m]."""
    sorted_cols, query_cols = _wide(sorted_cols), _wide(query_cols)
    if len(sorted_cols) != len(query_cols):
        raise ValueError("sorted and query tuples differ in width")
    if _native(query_cols[0], "lex_searchsorted"):
        return _C.lex_searchsorted(sorted_cols, query_cols, bool(right))
    # Dense lexicographic ranks of all tuples, then the scalar search:
    # equal tuples share a rank and the sorted side's ranks are sorted.
    u = sorted_cols[0].shape[0]
    both = [torch.cat([s, q]) for s, q in zip(sorted_cols, query_cols)]
    perm = lex_argsort(both)
    ordered = [c[perm] for c in both]
    step = torch.zeros(perm.shape[0], dtype=torch.int64,
                       device=perm.device)
    for c in ordered:
        step[1:] |= (c[1:] != c[:-1]).to(torch.int64)
    rank = torch.empty_like(step)
    rank[perm] = torch.cumsum(step, 0)
    return torch.searchsorted(rank[:u].contiguous(), rank[u:].contiguous(),
                              right=bool(right))


def merge_sorted_unique_multi(a_cols, b_cols):
    """Sorted-unique union of two lexicographically SORTED tuple sets:
    merge_sorted_unique's searchsorted scatter, over tuples."""
    a_cols, b_cols = list(a_cols), list(b_cols)
    n, m = a_cols[0].shape[0], b_cols[0].shape[0]
    dev = a_cols[0].device
    pos_a = (torch.arange(n, device=dev)
             + lex_searchsorted(b_cols, a_cols, right=False))
    pos_b = (torch.arange(m, device=dev)
             + lex_searchsorted(a_cols, b_cols, right=True))
    merged = []
    for a, b in zip(a_cols, b_cols):
        mc = torch.empty(n + m, dtype=a.dtype, device=dev)
        mc[pos_a] = a
        mc[pos_b] = b
        merged.append(mc)
    return unique_sorted_multi(merged)


def sort_pairs(keys, vcols):
    """Stable sort of the rows (keys, *vcols) by key: (sorted_keys,
    sorted_vcols).  Exactly one 8-byte value column rides the direct
    (key, value) radix sort; any other shape sorts a permutation and
    gathers each column once."""
    if not _native(keys, "sort_pairs"):
        perm = torch.argsort(keys, stable=True)
    elif len(vcols) == 1 and vcols[0].dtype.itemsize == 8:
        ks, vs = _C.radix_sort_kv(keys.contiguous(), vcols[0].contiguous())
        return ks, [vs]
    else:
        perm = _C.radix_argsort(keys.contiguous())
    return keys[perm], [v[perm] for v in vcols]


def segment_reduce(sorted_keys, vcols, codes, arm=None):
    """K16: reduce each value column over the runs of SORTED keys, by
    codes 0=sum 1=min 2=max: (unique_keys, [aggregates]).

    Two device arms.  "runs": boundaries come from ONE k_runs_sorted
    pass, reused across columns, and k_segreduce walks each run with one
    thread — exact for ints in any order.  "rocprim": reduce-by-key per
    column.  "runs" is taken when every column is int64 and no run is
    longer than SEGREDUCE_MAX_RUN: on skewed runs one thread would
    serialize, and float sums need reduce-by-key's fixed reduction tree,
    which makes them run-to-run reproducible.  `arm` forces one of the
    two, whatever the run lengths; None applies the rule."""
    if arm not in (None, "runs", "rocprim"):
        raise ValueError(f"segment_reduce: unknown arm {arm!r}")
    n = sorted_keys.shape[0]
    if not _native(sorted_keys, "segment_reduce"):
        uniq, starts, ends = runs(sorted_keys)
        m = uniq.shape[0]
        seg = torch.repeat_interleave(
            torch.arange(m, device=uniq.device), ends - starts)
        return uniq, [
            torch.empty_like(v[:m]).scatter_reduce_(
                0, seg, v, reduce=_SCATTER_OP[c], include_self=False)
            for v, c in zip(vcols, codes)]
    ks = sorted_keys.contiguous()
    if arm == "runs" or (arm is None and
                         all(v.dtype == torch.int64 for v in vcols)):
        uq, starts, cnt = _C.runs_sorted(ks)
        guard = _C.runs_guard(starts, cnt, n).cpu()  # one sync
        m, maxlen = int(guard[0]), int(guard[1])
        if arm == "runs" or maxlen <= SEGREDUCE_MAX_RUN:
            starts = starts[:m]
            return uq[:m], [
                _C.segment_reduce_runs(v.contiguous(), starts, n, c)
                for v, c in zip(vcols, codes)]
    outs = []
    for v, c in zip(vcols, codes):
        uq, aggs, cnt = _C.segment_reduce_sorted(ks, v.contiguous(), c)
        if not outs:
            m = int(cnt.item())  # the count is read once
            uniq = uq[:m]
        outs.append(aggs[:m])
    return uniq, outs


def sort_combine(keys, vcols, codes, arm=None):
    """Group rows by key and reduce each value column: sort_pairs, then
    segment_reduce.  Keys come back sorted."""
    return segment_reduce(*sort_pairs(keys, vcols), codes, arm)
