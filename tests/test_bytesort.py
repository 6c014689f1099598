"""Byte-order ranks of a BYTES column (K24) on CPU tensors, against
Python's sorted / bytes.__lt__, and the routing of Cogroup over keys
with BYTES columns."""

import random

import pytest
import torch

BYTES = "bytes"

_P40 = bytes(range(1, 41))  # a 40-byte common prefix


def nasty_rows():
    """About 3300 rows: the cases that can go wrong, each three times
    over, and 3000 random rows of 0 to 20 bytes over {0, 1, 97, 255},
    shuffled."""
    r14 = b"fourteen-bytes"
    assert len(r14) == 14
    special = [
        b"", b"a", b"a\0", b"a\0\0",          # a prefix sorts first
        b"\x7f", b"\x80", b"\xff",            # bytes are unsigned
        b"1234567", b"12345678", r14, r14 + b"!",  # lengths 7, 8, 14, 15
        r14 + b"\0",                          # a round boundary
        _P40, _P40 + b"\x01", _P40 + b"\x02",  # six rounds and more
    ]
    rng = random.Random(24)
    rows = special * 3
    for _ in range(3000):
        rows.append(bytes(rng.choice((0, 1, 97, 255))
                          for _ in range(rng.randrange(21))))
    rng.shuffle(rows)
    return rows + [b"the-end"]  # the last byte of data is a row's last


@pytest.fixture(scope="module")
def rows():
    return nasty_rows()


@pytest.fixture(scope="module")
def col(rows):
    from bigslice_amd.frame import BytesColumn
    return BytesColumn.from_list(rows)


def check_ranks(ranks, rows):
    """ranks order the rows exactly as bytes.__lt__ does."""
    ranks = ranks.tolist()
    assert len(ranks) == len(rows)
    by_rank = sorted(range(len(rows)), key=lambda i: (ranks[i], rows[i]))
    for a, b in zip(by_rank, by_rank[1:]):
        assert (ranks[a] < ranks[b]) == (rows[a] < rows[b])
        assert (ranks[a] == ranks[b]) == (rows[a] == rows[b])
    assert [rows[i] for i in by_rank] == sorted(rows)


def key_of(row, w):
    """The round key as the issue defines it, as a signed int64 with the
    top bit flipped."""
    part = row[7 * w:7 * w + 7]
    valid = len(part)
    key = int.from_bytes(part.ljust(7, b"\0"), "big") << 8 | valid
    key ^= 1 << 63
    return key - (1 << 64) if key >= (1 << 63) else key


def test_order_ranks_match_sorted(col, rows):
    check_ranks(col.order_ranks(), rows)


def test_argsort_is_the_stable_byte_order(col, rows):
    perm = col.argsort().tolist()
    want = sorted(range(len(rows)), key=lambda i: rows[i])  # stable
    assert perm == want


def test_on_a_zero_copy_slice(col, rows):
    part = col[5:-5]
    assert int(part.offsets[0]) != 0
    check_ranks(part.order_ranks(), rows[5:-5])
    want = sorted(range(len(rows) - 10), key=lambda i: rows[5 + i])
    assert part.argsort().tolist() == want


def test_distinct_ranks_take_the_rounds_the_prefix_needs(col, rows):
    from bigslice_amd.frame import BytesColumn
    from bigslice_amd.kernels import bytesort
    # correct on duplicates too
    check_ranks(bytesort.distinct_order_ranks(col), rows)
    distinct = sorted(set(rows), key=lambda r: (len(r), r))
    stats = {}
    ranks = bytesort.distinct_order_ranks(BytesColumn.from_list(distinct),
                                          stats)
    check_ranks(ranks, distinct)
    # 41 bytes decide the rows that share the 40-byte prefix: bytes
    # [35, 42) are round 5, the sixth
    assert 6 <= stats["rounds"] <= 40 // 7 + 2


def test_ranks_of_small_columns():
    from bigslice_amd.frame import BytesColumn
    for small in ([], [b""], [b"x"], [b"b", b"a"], [b"", b""],
                  [b"same"] * 5):
        c = BytesColumn.from_list(small)
        check_ranks(c.order_ranks(), small)
        assert c.argsort().tolist() == sorted(range(len(small)),
                                              key=lambda i: small[i])


@pytest.mark.parametrize("w", [0, 1, 2])
def test_round_keys_match_their_definition(col, rows, w):
    from bigslice_amd.kernels import bytesort
    n = len(rows)
    # the last row ends at the last byte of data
    assert int(col.offsets[-1]) == col.data.shape[0] and len(rows[-1]) > 0
    idx = list(range(n)) + [n - 1, 0, -1, n, n + 7]
    got = bytesort.round_keys(col, torch.tensor(idx, dtype=torch.int64), w)
    want = [key_of(rows[i] if 0 <= i < n else b"", w) for i in idx]
    assert got.tolist() == want
    # and on the slice, whose row numbers start over
    part = bytesort.round_keys(col[5:-5], torch.tensor(
        [0, 1, n - 11, n - 10], dtype=torch.int64), w)
    assert part.tolist() == [key_of(rows[5], w), key_of(rows[6], w),
                             key_of(rows[n - 6], w), key_of(b"", w)]


def test_round_keys_order_as_the_stretches_do(rows):
    keys = [(key_of(r, 0), r[:7]) for r in rows]
    for (ka, a), (kb, b) in zip(keys, keys[1:]):
        assert (ka < kb) == (a < b) and (ka == kb) == (a == b)


def test_refine_flags():
    from bigslice_amd.kernels import bytesort
    k7, k3 = key_of(b"abcdefg", 0), key_of(b"abc", 0)
    grp = torch.tensor([0, 0, 0, 0, 4, 4, 4, 7])
    key = torch.tensor([k3, k3, k7, k7, k7, k7 + 256, k7 + 256, k7])
    head, stay = bytesort.refine(grp, key)
    assert head.tolist() == [0, 0, 2, 0, 4, 5, 0, 7]
    # tied and unfinished: the two k7 of group 0, the two of group 4
    assert stay.tolist() == [False, False, True, True,
                             False, True, True, False]


# -- routing -----------------------------------------------------------------

def _cogroup(key_dts, val_dts=(torch.int64,), ndeps=2):
    import bigslice_amd as bs
    from bigslice_amd.schema import Schema

    def gen(shard, ctx):
        return iter(())
    schema = Schema(list(key_dts) + list(val_dts), len(key_dts))
    return bs.Cogroup(*[bs.ReaderFunc(2, gen, schema)
                        for _ in range(ndeps)])


@pytest.fixture
def _switches(monkeypatch):
    monkeypatch.delenv("BIGSLICE_COGROUP_BYTES", raising=False)
    monkeypatch.delenv("BIGSLICE_COGROUP_MULTIKEY", raising=False)
    return monkeypatch


@pytest.mark.parametrize("key_dts", [
    (BYTES,), (BYTES, torch.int64), (torch.int32, BYTES),
    (BYTES, BYTES, torch.int64)], ids=str)
def test_cogroup_takes_bytes_keys_on_the_device(_switches, key_dts):
    cg = _cogroup(key_dts)
    assert cg._device_shape_ok() and cg._device_eligible()
    cg = _cogroup(key_dts, val_dts=(torch.float32, torch.int32), ndeps=3)
    assert cg._device_shape_ok() and cg._device_eligible()
    _switches.setenv("BIGSLICE_COGROUP_BYTES", "0")
    assert cg._device_shape_ok() and not cg._device_eligible()


def test_cogroup_shapes_accept_bytes_keys(_switches):
    for key_dts in [(BYTES,), (BYTES, torch.int64), (torch.int32, BYTES)]:
        assert _cogroup(key_dts)._device_shape_ok()


def test_cogroup_keeps_other_shapes_on_the_host(_switches):
    from bigslice_amd.schema import OBJECT
    for key_dts, val_dts in [
            ((OBJECT,), (torch.int64,)),
            ((BYTES, OBJECT), (torch.int64,)),
            ((BYTES, torch.float32), (torch.int64,)),
            ((BYTES,), (BYTES,)),              # a BYTES value column
            ((BYTES,), (OBJECT,)),
            ((torch.int64, torch.int64), (BYTES,)),
            ((torch.int32,), (torch.int64,))]:  # a single int32 key
        cg = _cogroup(key_dts, val_dts)
        assert not cg._device_shape_ok(), (key_dts, val_dts)
        assert not cg._device_eligible(), (key_dts, val_dts)
    nine = _cogroup((BYTES,) + (torch.int64,) * 8)
    assert not nine._device_eligible()


def test_cogroup_shapes_accepted_before_are_still_accepted(_switches):
    for key_dts, val_dts in [
            ((torch.int64,), (torch.int64,)),
            ((torch.int64,), (torch.float32, torch.int32)),
            ((torch.int64, torch.int64), (torch.int64,)),
            ((torch.int32, torch.int64, torch.int32), (torch.float64,)),
            ((torch.int64,) * 8, (torch.int64,))]:
        assert _cogroup(key_dts, val_dts)._device_shape_ok()
    # the BYTES switch does not touch integer keys
    _switches.setenv("BIGSLICE_COGROUP_BYTES", "0")
    assert _cogroup((torch.int64,))._device_eligible()


# -- the device path's steps, on CPU tensors ----------------------------------

def _side(n, key_dts, words, seed):
    from bigslice_amd.frame import BytesColumn, Frame
    rng = random.Random(seed)
    cols = []
    for dt in key_dts:
        if dt == BYTES:
            cols.append(BytesColumn.from_list(
                [rng.choice(words) for _ in range(n)]))
        else:
            cols.append(torch.tensor(
                [rng.randrange(-3, 3) for _ in range(n)], dtype=dt))
    cols.append(torch.arange(n))
    return Frame(cols, len(key_dts))


@pytest.mark.parametrize("key_dts", [
    (BYTES,), (BYTES, torch.int64), (torch.int32, BYTES)], ids=str)
def test_cogroup_steps_give_the_host_paths_rows_in_its_order(rows, key_dts):
    """_device_gen_bytes over CPU tensors (every step runs its torch
    form) against the host generator: the same keys in the same order,
    the same values per key and dep.  Three deps, one of them empty."""
    import types
    words = sorted(set(rows))[::11]
    nk = len(key_dts)
    cg = _cogroup(key_dts, ndeps=3)
    a, b = _side(4000, key_dts, words, 1), _side(3000, key_dts, words, 2)
    ctx = types.SimpleNamespace(device="cpu", chunk=1000)
    got = [r for f in cg._device_gen_bytes(
        [[a], [b.slice(0, 1500), b.slice(1500, 3000)], []], ctx)
        for r in f.rows()]
    want = [r for f in cg.reader(0, [[a], [b], []], ctx) for r in f.rows()]
    assert len(want) >= len(words)
    assert [r[:nk] for r in got] == [r[:nk] for r in want]
    assert ([tuple(sorted(v) for v in r[nk:]) for r in got]
            == [tuple(sorted(v) for v in r[nk:]) for r in want])
