"""Device Reduce over composite keys with BYTES columns (K23): the
aggregator on the device against a Python dict, and Reduce end to end
against a CPU session.  float32 inputs are small integers, so every
summation order gives the same float."""

import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BYTES = "bytes"

_ORDERS = {
    "bytes_int": [BYTES, torch.int64],
    "int_bytes": [torch.int64, BYTES],
    "bytes_bytes": [BYTES, BYTES],
    "int32_bytes_int64": [torch.int32, BYTES, torch.int64],
}

_NWORDS = 700
_WORDS = [b"", b"a", b"aa"] + [b"term-%d" % i for i in range(_NWORDS - 3)]


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    for name in ("BIGSLICE_GB_FP_BITS", "BIGSLICE_GB_MULTIKEY",
                 "BIGSLICE_GB_BYTES_MULTIKEY"):
        monkeypatch.delenv(name, raising=False)


def _stat(name):
    from bigslice_amd.utils import stats
    return stats.DEFAULT.values().get(name, 0)


_BATCHES = {}


def _batches(order):
    """Three batches, 200,000 rows in all over about 20,000 tuples:
    [(key columns: index tensors into _WORDS or integers, int64 values,
    float32 values)], built once per key order."""
    if order in _BATCHES:
        return _BATCHES[order]
    key_dts = _ORDERS[order]
    # the cardinality of every key column, about 20,000 tuples in all
    nb = sum(dt == BYTES for dt in key_dts)
    cards = []
    for dt in key_dts:
        if dt == BYTES:
            cards.append(_NWORDS if nb == 1 else 141)
        else:
            cards.append(29 if len(key_dts) == 2 else 5)
    g = torch.Generator().manual_seed(len(order))
    out = []
    for n in (120_000, 50_000, 30_000):
        keys = [torch.randint(0, c, (n,), generator=g) for c in cards]
        ints = torch.randint(-1000, 1000, (n,), generator=g)
        floats = torch.randint(-8, 9, (n,), generator=g).to(torch.float32)
        out.append((keys, ints, floats))
    _BATCHES[order] = out
    return out


def _key_value(idx, dt):
    return _WORDS[idx] if dt == BYTES else idx - 2


def _oracle(order, aggs):
    key_dts = _ORDERS[order]
    fns = {"sum": lambda a, b: a + b, "min": min, "max": max}
    state = {}
    for keys, ints, floats in _batches(order):
        cols = [[_key_value(i, dt) for i in k.tolist()]
                for k, dt in zip(keys, key_dts)]
        for row in zip(*cols, ints.tolist(), floats.tolist()):
            k, v = row[:len(key_dts)], row[len(key_dts):]
            cur = state.get(k)
            if cur is None:
                state[k] = list(v)
            else:
                for j, a in enumerate(aggs):
                    cur[j] = fns[a](cur[j], v[j])
    return {k: tuple(v) for k, v in state.items()}


def _frames(order):
    from bigslice_amd.frame import BytesColumn, Frame
    key_dts = _ORDERS[order]
    words = BytesColumn.from_list(_WORDS, DEV)
    for keys, ints, floats in _batches(order):
        cols = []
        for k, dt in zip(keys, key_dts):
            if dt == BYTES:
                cols.append(words.select(k.to(DEV)))
            else:
                cols.append((k - 2).to(dt).to(DEV))
        yield Frame(cols + [ints.to(DEV), floats.to(DEV)], len(key_dts))


def _run(order, aggs):
    from bigslice_amd.frame import BytesColumn
    from bigslice_amd.ops.aggregate import (Aggregation,
                                            BytesTupleAggregator,
                                            make_aggregator)
    from bigslice_amd.schema import Schema
    key_dts = _ORDERS[order]
    schema = Schema(key_dts + [torch.int64, torch.float32], len(key_dts))
    a = make_aggregator(schema, Aggregation(aggs), DEV)
    assert isinstance(a, BytesTupleAggregator)
    for f in _frames(order):
        a.add(f)
    got = {}
    for f in a.result_frames(7001):
        assert len(f) <= 7001 and f.combined_id is not None
        for c, dt in zip(f.columns[:len(key_dts)], key_dts):
            if dt == BYTES:
                assert isinstance(c, BytesColumn) and c.data.is_cuda
            else:
                assert c.dtype == dt and c.is_cuda
        assert f.columns[-2].dtype == torch.int64
        assert f.columns[-1].dtype == torch.float32
        for row in f.rows():
            k = row[:len(key_dts)]
            assert k not in got
            got[k] = row[len(key_dts):]
    return got


@pytest.mark.parametrize("order", sorted(_ORDERS))
def test_device_aggregator_against_a_dict(kernels, order):
    want = _oracle(order, ["sum", "sum"])
    assert 15_000 < len(want) < 25_000
    before = _stat("combiner/bytes_tuple_tables")
    fallbacks = _stat("combiner/fingerprint_fallbacks")
    assert _run(order, ["sum", "sum"]) == want
    assert _stat("combiner/bytes_tuple_tables") == before + 1
    assert _stat("combiner/fingerprint_fallbacks") == fallbacks


def test_device_aggregator_min_max(kernels):
    want = _oracle("bytes_int", ["min", "max"])
    assert _run("bytes_int", ["min", "max"]) == want


def test_narrow_fingerprint_falls_back_exactly(kernels, monkeypatch):
    """About 20,000 tuples cannot have different 4-bit tags."""
    monkeypatch.setenv("BIGSLICE_GB_FP_BITS", "4")
    want = _oracle("int32_bytes_int64", ["sum", "sum"])
    before = _stat("combiner/fingerprint_fallbacks")
    assert _run("int32_bytes_int64", ["sum", "sum"]) == want
    assert _stat("combiner/fingerprint_fallbacks") == before + 1


def test_routing_on_a_gpu_device(kernels, monkeypatch):
    from bigslice_amd.ops.aggregate import (Aggregation, BytesKeyAggregator,
                                            BytesTupleAggregator,
                                            DictAggregator, make_aggregator)
    from bigslice_amd.schema import Schema
    agg = Aggregation(["sum"])
    pair = Schema([BYTES, torch.int64, torch.int64], 2)
    assert isinstance(make_aggregator(pair, agg, DEV), BytesTupleAggregator)
    one = Schema([BYTES, torch.int64], 1)
    assert isinstance(make_aggregator(one, agg, DEV), BytesKeyAggregator)
    fl = Schema([BYTES, torch.float32, torch.int64], 2)
    assert isinstance(make_aggregator(fl, agg, DEV), DictAggregator)
    monkeypatch.setenv("BIGSLICE_GB_BYTES_MULTIKEY", "0")
    assert isinstance(make_aggregator(pair, agg, DEV), DictAggregator)


# -- end to end --------------------------------------------------------------

def _reduce_rows(device):
    import bigslice_amd as bs
    from bigslice_amd.frame import BytesColumn
    g = torch.Generator().manual_seed(8)
    n = 40_000
    words = [_WORDS[i] for i in
             torch.randint(0, 300, (n,), generator=g).tolist()]
    docs = torch.randint(-20, 20, (n,), dtype=torch.int64, generator=g)
    v = torch.randint(-1000, 1000, (n,), dtype=torch.int64, generator=g)
    nshard = 8

    def gen(shard, ctx):
        sel = torch.arange(shard, n, nshard)
        col = BytesColumn.from_list([words[i] for i in sel.tolist()],
                                    ctx.device)
        yield (col, docs[sel].to(ctx.device), v[sel].to(ctx.device))

    def job():
        src = bs.ReaderFunc(nshard, gen, bs.schema_of(bytes, int, int))
        return bs.Reduce(bs.Prefixed(src, 2), "sum")
    sess = bs.start(parallelism=2, device=device)
    rows = sorted((bytes(w), int(d), int(c))
                  for w, d, c in sess.run(bs.func(job)).scan())
    sess.shutdown()
    return rows


def test_reduce_over_a_bytes_and_int_prefix(kernels, monkeypatch):
    want = _reduce_rows("cpu")
    assert len(want) > 5000
    tables = _stat("combiner/bytes_tuple_tables")
    got = _reduce_rows(DEV)
    assert got == want
    ran = _stat("combiner/bytes_tuple_tables")
    assert ran > tables, "the composite BYTES key path did not run"
    monkeypatch.setenv("BIGSLICE_GB_BYTES_MULTIKEY", "0")
    assert _reduce_rows(DEV) == want
    assert _stat("combiner/bytes_tuple_tables") == ran


def test_device_term_counts(kernels):
    import bigslice_amd as bs
    from bigslice_amd import recipes
    g = torch.Generator().manual_seed(21)
    lines, want = [], collections.Counter()
    for i in range(2000):
        doc = i % 37
        idx = torch.randint(3, 200, (int(torch.randint(0, 12, (1,),
                                                       generator=g)),),
                            generator=g).tolist()
        toks = [_WORDS[j] for j in idx]
        lines.append("%d\t%s" % (doc, b"  ".join(toks).decode()))
        want.update((t, doc) for t in toks)
    tables = _stat("combiner/bytes_tuple_tables")
    sess = bs.start(parallelism=2, device=DEV)
    res = sess.run(bs.func(
        lambda: recipes.device_term_counts(4, lambda: iter(lines))))
    got = {(bytes(w), int(d)): int(c) for w, d, c in res.scan()}
    sess.shutdown()
    assert got == dict(want)
    assert _stat("combiner/bytes_tuple_tables") > tables
