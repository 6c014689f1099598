"""Device kernel dispatch.

Loads the in-tree HIP extension (bigslice_amd._C, built by setup.py for
gfx950).  Policy: on a GPU host the extension MUST be present — device ops
raise rather than silently falling back to eager torch, so a missing build
is loud.  On CPU-only hosts everything falls back to torch/numpy reference
implementations (used by tests as numerics oracles).
"""

from __future__ import annotations

import os
from typing import List, Optional

import torch

_C = None
_load_error: Optional[BaseException] = None

try:
    from bigslice_amd import _C as _C  # built by setup.py build_ext --inplace
except Exception as e:  # pragma: no cover
    _load_error = e


ALLOW_FALLBACK = os.environ.get("BIGSLICE_ALLOW_EAGER_FALLBACK", "0") == "1"


def have_extension() -> bool:
    return _C is not None


def _require(feature: str):
    if _C is None:
        raise RuntimeError(
            f"bigslice_amd._C extension not available for {feature} on a "
            f"GPU tensor (build with `python setup.py build_ext --inplace`); "
            f"import error: {_load_error!r}")


def native(on_gpu: bool, feature: str) -> bool:
    """The extension gate: whether `feature` runs in the extension.  True
    with the extension loaded and the input on a GPU.  Without it, an
    input on a GPU raises (no silent eager fallback) unless
    BIGSLICE_ALLOW_EAGER_FALLBACK=1; everything else takes the torch
    path.  The flag and the module are looked up on every call."""
    if _C is not None:
        return bool(on_gpu)
    if on_gpu and not ALLOW_FALLBACK:
        _require(feature)
    return False


# -- hashing --------------------------------------------------------------

def hash_columns_device(cols: List[torch.Tensor], seed: int) -> torch.Tensor:
    """murmur3-32 XOR-combined over key columns; returns uint32 tensor."""
    if not native(True, "hash_columns"):
        from .. import hashing
        host = [c.cpu() for c in cols]
        return hashing.hash_columns(host, seed).to(cols[0].device)
    return _C.hash_columns(cols, seed)


# -- partition (K4) -------------------------------------------------------

def partition_supported(frame) -> bool:
    # (asked only of frames of a GPU session)
    return native(True, "partition_frame") and all(
        isinstance(c, torch.Tensor) for c in frame.columns)


def partition_frame(frame, num_partitions: int, partitioner):
    """Fused hash+histogram+scatter: returns per-partition sub-frames
    (views over one reordered buffer)."""
    from ..frame import Frame
    if partitioner is not None:
        p = partitioner(frame, num_partitions).to(torch.int32)
        reordered_cols, counts = _C.scatter_by_partition(
            list(frame.columns), p, num_partitions)
    else:
        key_cols = list(frame.columns[: frame.prefix])
        reordered_cols, counts = _C.hash_partition(
            list(frame.columns), key_cols, num_partitions, 0)
    # partitioning preserves row identity: a unique-keyed (combined)
    # input stays unique per partition
    sorted_f = Frame(reordered_cols, frame.prefix,
                     combined_id=frame.combined_id)
    out = []
    off = 0
    for c in counts.tolist():
        out.append(sorted_f.slice(off, off + c) if c else None)
        off += c
    return out


# -- group-by aggregate (K9) ----------------------------------------------

# (kernels.groupby is the function, as ever: reach the module's other
# names with `from bigslice_amd.kernels.groupby import ...`)
from .groupby import (  # noqa: E402,F401
    _AGG_CODES, _GB_KEY_DTYPES, _GB_VAL_DTYPES, GB_SENTINEL, MAX_PROBES,
    PART_LDS_SLOTS, PART_MAX_BUCKETS, PART_OWN_LIMIT, PART_TILE_ROWS,
    GroupTable, _next_pow2, groupby, groupby_shape_supported,
    groupby_supported, part_buckets, part_owned_buckets)

# -- group-by aggregate over multi-column integer keys (K21) ---------------

from .groupby_multi import MultiKeyTable, fingerprint64  # noqa: E402,F401

# -- id dictionary and varlen row gather for BYTES key columns (K23) -------

from .iddict import IdDictionary, bytes_gather  # noqa: E402,F401

# -- byte-order ranks of a BYTES column (K24) ------------------------------

from .bytesort import (  # noqa: E402,F401
    distinct_order_ranks, order_ranks, round_keys)


# -- sort (K6) -------------------------------------------------------------

def sort_pairs_supported(keys: torch.Tensor) -> bool:
    return _C is not None and keys.dtype in (torch.int64, torch.int32,
                                             torch.float32, torch.float64)


def radix_argsort(keys: torch.Tensor) -> torch.Tensor:
    """Device radix sort; returns the sorting permutation (int64)."""
    if not native(keys.is_cuda, "radix_argsort"):
        return torch.argsort(keys, stable=True)
    return _C.radix_argsort(keys)


def radix_sort_kv(keys: torch.Tensor, val: torch.Tensor):
    """Direct (key, value) radix sort for one 8-byte value column."""
    if not native(keys.is_cuda, "radix_sort_kv"):
        perm = torch.argsort(keys, stable=True)
        return keys[perm], val[perm]
    v64 = val.view(torch.int64) if val.dtype != torch.int64 else val
    sk, sv = _C.radix_sort_kv(keys, v64)
    return sk, (sv.view(val.dtype) if val.dtype != torch.int64 else sv)


def radix_sort_keys(keys: torch.Tensor) -> torch.Tensor:
    """Device radix key-only sort (no permutation)."""
    if not native(keys.is_cuda, "radix_sort_keys"):
        return torch.sort(keys).values
    return _C.radix_sort_keys(keys)


# -- fused Map/Filter expressions (K13) -------------------------------------

# rows per tile of the expression kernel (csrc/expr.hip: 256 x 32)
EXPR_TILE_ROWS = 8192

_EXPR_DTYPES = (torch.bool, torch.int32, torch.int64, torch.float32,
                torch.float64)


def expr_supported(program, frame) -> bool:
    """True when expr_apply can run this (native-eligible) program on
    this frame: every column it reads or writes is a dense contiguous
    device tensor of a vocabulary dtype.  Pass-through columns of a
    predicate-free program are not touched and may be anything."""
    cols = [frame.columns[i] for i in program.inputs]
    on_gpu = any(isinstance(c, torch.Tensor) and c.is_cuda
                 for c in frame.columns)
    if not native(on_gpu, "expr_apply"):
        return False
    # (a column whose dtype is not the schema's the program was typed
    # from also takes the eval path, where torch promotes what it sees)
    return program.eligible and all(
        isinstance(c, torch.Tensor) and c.is_cuda and c.dim() == 1
        and c.is_contiguous() and c.dtype in _EXPR_DTYPES and c.dtype == dt
        for c, dt in zip(cols, program.in_dtypes))


def expr_apply(program, cols):
    """Run a compiled expression program (exprs.compile_program) over
    the frame columns ``cols`` in one kernel launch.  Returns
    (out_cols, count): count is None without a predicate; with one, the
    outputs hold the ``count`` surviving rows in input order."""
    from ..exprs import _DT_CODE
    _require("expr_apply")
    ins = [cols[i] for i in program.inputs]
    regs = [v for kind, v in program.outputs if kind == "reg"]
    dts = [_DT_CODE[dt] for (kind, _), dt in
           zip(program.outputs, program.out_dtypes) if kind == "reg"]
    has_pred = program.pred_reg >= 0
    n = ins[0].shape[0] if ins else 0
    if n == 0 or not regs:
        # nothing to launch: an empty batch, or only pass-through columns
        outs = [torch.empty(0, dtype=dt, device=ins[0].device)
                for (kind, _), dt in zip(program.outputs,
                                         program.out_dtypes)
                if kind == "reg"]
        res = iter(outs)
        return ([next(res) if kind == "reg" else cols[v]
                 for kind, v in program.outputs],
                0 if has_pred else None)
    got = _C.expr_apply(program.code(), program.n_pred, program.pred_reg,
                        ins, regs, dts)
    count = None
    if has_pred:
        count = int(got.pop().item())  # the one readback per batch
        # a selective filter must not pin the n-row allocation: at most
        # 2x its own bytes stay referenced
        got = [o[:count].clone() if 2 * count <= n else o[:count]
               for o in got]
    res = iter(got)
    return ([next(res) if kind == "reg" else cols[v]
             for kind, v in program.outputs], count)


# -- device tokenizer (K20) --------------------------------------------------

# bytes per tile of the tokenizer kernels (csrc/tokenize.hip)
TOKENIZE_TILE_BYTES = _C.TOKENIZE_TILE_BYTES if _C is not None else 16384

# bytes.split()'s whitespace (ASCII only; str.split() also splits on
# Unicode spaces, which this set does not contain)
ASCII_WHITESPACE = b" \t\n\r\x0b\x0c"


def tokenize_mask(delims=None) -> List[int]:
    """The 256-bit delimiter set as four uint64 words: bit (b & 63) of
    word (b >> 6) is set iff byte b is a delimiter.  None means ASCII
    whitespace; an empty set raises ValueError."""
    if delims is None:
        delims = ASCII_WHITESPACE
    if isinstance(delims, str):
        raise TypeError("delims must be bytes, not str")
    delims = bytes(delims)
    if not delims:
        raise ValueError("empty delimiter set")
    words = [0, 0, 0, 0]
    for b in delims:
        words[b >> 6] |= 1 << (b & 63)
    return words


def tokenize_bytes(data: torch.Tensor, offsets: torch.Tensor, mask4,
                   with_rows: bool = False):
    """Split the rows of a compacted device BYTES column (zero-based
    offsets, data.numel() == offsets[-1] < 2^31) into tokens on the HIP
    kernels.  Returns (out_data, out_offsets) or, with_rows,
    (out_data, out_offsets, tok_row).  One host readback (the totals)."""
    _require("tokenize_bytes")
    return tuple(_C.tokenize_bytes(data, offsets, list(mask4),
                                   bool(with_rows)))
