"""Operations on key-sorted arrays: run boundaries (K18), the
sorted-unique merge, their multi-column forms with a lexicographic
sort and search (K22), and the sort-combine pipeline (K6 sort + K16
segmented reduction).

Every function takes and returns torch tensors.  A device tensor goes to
the HIP extension; a CPU tensor runs a torch implementation that gives
the same result — the contract the device path is tested against.
"""

import torch

from .. import kernels as _k
from . import _C, native

SEGREDUCE_MAX_RUN = 4096  # longest run k_segreduce takes, a thread per run
# scatter_reduce_'s name of an aggregation, by code (groupby._AGG_CODES)
_SCATTER_OP = ("sum", "amin", "amax", "prod")

# A key is a tuple of 1 to MAX_KEY_COLS integer columns, first column
# most significant; the functions of one key array are the one-column
# case.  One device int64 column runs the K18 pass (_C.runs_sorted) and
# torch.searchsorted, never the tuple kernels: their one-column
# instantiation is the generic 8-column one.  With two or more columns
# the extension takes contiguous int64: int32 columns are widened on the
# way in and narrowed on the way out, as MultiKeyTable does.

# rows per tile of the run-boundary kernels (csrc/runs_multi.hip)
MRUNS_TILE_ROWS = _C.MRUNS_TILE_ROWS if _C is not None else 4096


def _wide(cols):
    return [c.to(torch.int64).contiguous() for c in cols]


def lex_argsort(cols):
    """Stable permutation sorting the rows of `cols` lexicographically:
    one stable sort per column from the last to the first (device: the
    radix argsort, stable on both of its engines; CPU: torch.sort)."""
    cols = list(cols)
    on_dev = native(cols[0].is_cuda, "lex_argsort")
    perm = None
    for c in reversed(cols):
        k = c if perm is None else c[perm]
        if on_dev:
            o = _k._C.radix_argsort(k.contiguous())
        else:
            o = torch.sort(k, stable=True).indices
        perm = o if perm is None else perm[o]
    return perm


def lex_sort_keys(cols):
    """The key tuples of `cols` in lexicographic order, keys only (one
    column: the key-only radix sort)."""
    if len(cols) == 1:
        from . import radix_sort_keys
        return [radix_sort_keys(cols[0])]
    perm = lex_argsort(cols)
    return [c[perm] for c in cols]


def _uniq_starts(sorted_cols):
    """([distinct tuples per column], run_starts) of lexicographically
    SORTED columns, one readback.  One device int64 column: ONE pass
    (_C.runs_sorted, 8 B/row read); two or more device columns:
    _C.runs_multi; otherwise diff mask + nonzero + gather (3 reads of
    the key arrays + a bool-mask round trip)."""
    first = sorted_cols[0]
    n = first.shape[0]
    if len(sorted_cols) == 1:
        if n and first.dtype == torch.int64 and native(first.is_cuda, "runs"):
            uniq, starts, cnt = _k._C.runs_sorted(first.contiguous())
            c = int(cnt.item())
            return [uniq[:c]], starts[:c]
    elif n and native(first.is_cuda, "runs_multi"):
        uniq, starts, cnt = _k._C.runs_multi(_wide(sorted_cols))
        c = int(cnt.item())
        return ([u[:c] if s.dtype == torch.int64 else u[:c].to(s.dtype)
                 for u, s in zip(uniq, sorted_cols)], starts[:c])
    mask = torch.ones(n, dtype=torch.bool, device=first.device)
    mask[1:] = first[1:] != first[:-1]
    for c in sorted_cols[1:]:
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
    uniq, starts = _uniq_starts(sorted_cols)
    ends = torch.cat([starts[1:],
                      torch.tensor([n], dtype=torch.int64, device=dev)])
    return uniq, starts, ends


def unique_sorted_multi(sorted_cols):
    """The distinct tuples of lexicographically SORTED columns, in order,
    one tensor per column."""
    sorted_cols = list(sorted_cols)
    if len(sorted_cols) == 1:
        return _uniq_starts(sorted_cols)[0]
    # Tuples keep K22's launches, the `ends` that runs_multi builds and
    # nobody reads included (a cat and a one-element copy per call);
    # dropping them is a change of its own, with its own trace.
    return runs_multi(sorted_cols)[0]


def lex_searchsorted(sorted_cols, query_cols, right=False):
    """torch.searchsorted over tuples: for every query tuple, the first
    position among the lexicographically SORTED tuples whose tuple is
    >= the query (right=False) or > the query (right=True).  int64[m]."""
    if len(sorted_cols) != len(query_cols):
        raise ValueError("sorted and query tuples differ in width")
    if len(sorted_cols) == 1:
        return torch.searchsorted(sorted_cols[0], query_cols[0],
                                  right=bool(right))
    sorted_cols, query_cols = _wide(sorted_cols), _wide(query_cols)
    if native(query_cols[0].is_cuda, "lex_searchsorted"):
        return _k._C.lex_searchsorted(sorted_cols, query_cols, bool(right))
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
    """Sorted-unique union of two lexicographically SORTED tuple sets via
    searchsorted scatter (2 passes; ~3x cheaper than re-sorting the
    concatenation)."""
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


def runs(sorted_keys):
    """(unique_keys, starts, ends) of the runs of a SORTED key array."""
    uniq, starts, ends = runs_multi([sorted_keys])
    return uniq[0], starts, ends


def unique_sorted(sorted_keys):
    """The distinct keys of a SORTED array, in order."""
    return unique_sorted_multi([sorted_keys])[0]


def merge_sorted_unique(a, b):
    """Sorted-unique union of two SORTED key arrays."""
    return merge_sorted_unique_multi([a], [b])[0]


def sort_pairs(keys, vcols):
    """Stable sort of the rows (keys, *vcols) by key: (sorted_keys,
    sorted_vcols).  Exactly one 8-byte value column rides the direct
    (key, value) radix sort; any other shape sorts a permutation and
    gathers each column once."""
    if not native(keys.is_cuda, "sort_pairs"):
        perm = torch.argsort(keys, stable=True)
    elif len(vcols) == 1 and vcols[0].dtype.itemsize == 8:
        ks, vs = _k._C.radix_sort_kv(keys.contiguous(),
                                     vcols[0].contiguous())
        return ks, [vs]
    else:
        perm = _k._C.radix_argsort(keys.contiguous())
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
    if not native(sorted_keys.is_cuda, "segment_reduce"):
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
        uq, starts, cnt = _k._C.runs_sorted(ks)
        guard = _k._C.runs_guard(starts, cnt, n).cpu()  # one sync
        m, maxlen = int(guard[0]), int(guard[1])
        if arm == "runs" or maxlen <= SEGREDUCE_MAX_RUN:
            starts = starts[:m]
            return uq[:m], [
                _k._C.segment_reduce_runs(v.contiguous(), starts, n, c)
                for v, c in zip(vcols, codes)]
    outs = []
    for v, c in zip(vcols, codes):
        uq, aggs, cnt = _k._C.segment_reduce_sorted(ks, v.contiguous(), c)
        if not outs:
            m = int(cnt.item())  # the count is read once
            uniq = uq[:m]
        outs.append(aggs[:m])
    return uniq, outs


def sort_combine(keys, vcols, codes, arm=None):
    """Group rows by key and reduce each value column: sort_pairs, then
    segment_reduce.  Keys come back sorted."""
    return segment_reduce(*sort_pairs(keys, vcols), codes, arm)
