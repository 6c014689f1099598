"""Composite keys with BYTES columns (K23), without a GPU: the routing
of make_aggregator, BytesTupleAggregator on "cpu" (the host mirror of
the id dictionary over a TensorAggregator of ids), IdDictionary on CPU
tensors and BytesColumn.gather on a host column.

Oracles are Python dicts and BytesColumn.select, never the code under
test."""

import pytest
import torch

from bigslice_amd.frame import BytesColumn, Frame
from bigslice_amd.kernels.groupby import GB_SENTINEL
from bigslice_amd.kernels.iddict import IdDictionary
from bigslice_amd.ops.aggregate import (Aggregation, BytesKeyAggregator,
                                        BytesTupleAggregator, DictAggregator,
                                        make_aggregator)
from bigslice_amd.schema import Schema

BYTES = "bytes"

# b"", prefixes of one another, and strings that differ in the last byte
WORDS = [b"", b"a", b"aa", b"aaa", b"ab", b"prefix-0", b"prefix-1",
         b"prefix-2", b"x" * 40 + b"y", b"x" * 40 + b"z"]


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    monkeypatch.delenv("BIGSLICE_GB_BYTES_MULTIKEY", raising=False)


# -- routing ---------------------------------------------------------------

def test_cpu_session_keeps_the_dict():
    schema = Schema([BYTES, torch.int64, torch.int64], 2)
    agg = make_aggregator(schema, Aggregation(["sum"]), "cpu")
    assert isinstance(agg, DictAggregator)


def test_one_bytes_key_keeps_its_aggregator():
    schema = Schema([BYTES, torch.int64], 1)
    agg = make_aggregator(schema, Aggregation(["sum"]), "cpu")
    assert isinstance(agg, BytesKeyAggregator)


def test_float_key_and_nine_columns_go_to_the_dict():
    from bigslice_amd.ops.aggregate import bytes_tuple_supported
    agg = Aggregation(["sum"])
    fl = Schema([BYTES, torch.float32, torch.int64], 2)
    nine = Schema([BYTES] + [torch.int64] * 9, 9)
    for schema in (fl, nine):
        assert not bytes_tuple_supported(schema, agg)
        assert isinstance(make_aggregator(schema, agg, "cpu"),
                          DictAggregator)
        with pytest.raises(ValueError):
            BytesTupleAggregator(schema, agg, "cpu")
    ok = Schema([BYTES, torch.int32, torch.int64], 2)
    assert bytes_tuple_supported(ok, agg)
    assert not bytes_tuple_supported(ok, Aggregation([lambda a, b: a]))
    assert not bytes_tuple_supported(Schema([BYTES, torch.int64], 1), agg)


# -- BytesTupleAggregator on the CPU ----------------------------------------

_ORDERS = {
    "bytes_int": [BYTES, torch.int64],
    "int_bytes": [torch.int64, BYTES],
    "bytes_bytes": [BYTES, BYTES],
    "int32_bytes_int64": [torch.int32, BYTES, torch.int64],
}

_PY_AGG = {"sum": lambda a, b: a + b, "min": min, "max": max}


def _batches(key_dts, sizes, seed):
    """[(key columns as Python lists, values)] for each batch size."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        keys = []
        for dt in key_dts:
            if dt == BYTES:
                idx = torch.randint(0, len(WORDS), (n,), generator=g)
                keys.append([WORDS[i] for i in idx.tolist()])
            else:
                keys.append(torch.randint(-3, 4, (n,), generator=g).tolist())
        vals = torch.randint(-1000, 1000, (n,), generator=g).tolist()
        out.append((keys, vals))
    return out


def _frame(keys, vals, key_dts, device="cpu"):
    cols = []
    for k, dt in zip(keys, key_dts):
        if dt == BYTES:
            cols.append(BytesColumn.from_list(k, device))
        else:
            cols.append(torch.tensor(k, dtype=dt, device=device))
    cols.append(torch.tensor(vals, dtype=torch.int64, device=device))
    return Frame(cols, len(key_dts))


def _oracle(batches, agg):
    fn = _PY_AGG[agg]
    state = {}
    for keys, vals in batches:
        for row in zip(*keys, vals):
            k, v = row[:-1], row[-1]
            state[k] = fn(state[k], v) if k in state else v
    return state


@pytest.mark.parametrize("agg", ["sum", "min", "max"])
@pytest.mark.parametrize("order", sorted(_ORDERS))
def test_cpu_aggregator_against_a_dict(order, agg):
    key_dts = _ORDERS[order]
    batches = _batches(key_dts, [700, 0, 301], seed=len(order))
    schema = Schema(key_dts + [torch.int64], len(key_dts))
    a = BytesTupleAggregator(schema, Aggregation([agg]), "cpu")
    for keys, vals in batches:
        a.add(_frame(keys, vals, key_dts))
    got = {}
    for f in a.result_frames(97):
        assert len(f) <= 97
        assert f.prefix == len(key_dts)
        for c, dt in zip(f.columns, key_dts):
            if dt == BYTES:
                assert isinstance(c, BytesColumn)
            else:
                assert c.dtype == dt
        for row in f.rows():
            assert row[:-1] not in got
            got[row[:-1]] = row[-1]
    assert got == _oracle(batches, agg)


def test_cpu_aggregator_with_no_rows():
    schema = Schema([BYTES, torch.int64, torch.int64], 2)
    a = BytesTupleAggregator(schema, Aggregation(["sum"]), "cpu")
    a.add(_frame([[], []], [], [BYTES, torch.int64]))
    assert list(a.result_frames(10)) == []


# -- IdDictionary on CPU tensors ---------------------------------------------

def _check_dictionary(d, cols_ids):
    """Every row of every added column resolves to its own bytes."""
    strings = d.strings().tolists()
    assert len(strings) == len(d)
    distinct = set()
    for col, ids in cols_ids:
        pos = d.lookup(ids).tolist()
        rows = col.tolists()
        assert all(0 <= p < len(d) for p in pos)
        assert [strings[p] for p in pos] == rows
        distinct.update(rows)
    assert len(d) == len(distinct)


def test_cpu_dictionary_contract():
    g = torch.Generator().manual_seed(5)
    d = IdDictionary("cpu")
    added = []
    for n in (500, 0, 300):
        idx = torch.randint(0, len(WORDS), (n,), generator=g).tolist()
        col = BytesColumn.from_list([WORDS[i] for i in idx])
        ids = col.ids64()
        d.add(ids, col)
        added.append((col, ids))
    _check_dictionary(d, added)
    assert len(d) == len(WORDS)
    absent = BytesColumn.from_list([b"not there"]).ids64()
    assert d.lookup(absent).tolist() == [-1]
    # a batch added twice adds nothing
    before = d.strings().tolists()
    d.add(added[0][1], added[0][0])
    assert len(d) == len(WORDS)
    assert d.strings().tolists() == before


def test_cpu_dictionary_empty_marker_is_id_zero():
    col = BytesColumn.from_list([b"same", b"same", b"other"])
    ids = torch.tensor([GB_SENTINEL, 0, 7], dtype=torch.int64)
    d = IdDictionary("cpu")
    d.add(ids, col)
    assert len(d) == 2
    pos = d.lookup(ids).tolist()
    assert pos[0] == pos[1] != pos[2]
    strings = d.strings().tolists()
    assert [strings[p] for p in pos] == col.tolists()


def test_empty_dictionary():
    d = IdDictionary("cpu")
    assert len(d) == 0 and len(d.strings()) == 0
    assert d.lookup(torch.tensor([1, 2])).tolist() == [-1, -1]


# -- BytesColumn.gather on the CPU --------------------------------------------

def test_gather_on_the_cpu_is_select():
    col = BytesColumn.from_list(WORDS * 3)
    idx = torch.tensor([29, 0, 0, 5, 17, 1, 9], dtype=torch.int64)
    for c in (col, col[3:25]):
        i = idx % len(c)
        got, want = c.gather(i), c.select(i)
        assert torch.equal(got.data, want.data)
        assert torch.equal(got.offsets, want.offsets)
    empty = col.gather(torch.empty(0, dtype=torch.int64))
    assert len(empty) == 0 and empty.data.numel() == 0
