"""The two device primitives of K23: the variable-length row gather
(csrc/bytes_gather.hip) against BytesColumn.select, and the id
dictionary (csrc/iddict.hip) against its contract: every id of every
added row resolves to a position whose bytes equal that row's bytes."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


def _column(rows, device=DEV):
    from bigslice_amd.frame import BytesColumn
    return BytesColumn.from_list(rows, device)


def _rand_rows(n, lo, hi, seed):
    """n rows of lo..hi random bytes each."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, hi + 1, (n,), generator=g).tolist()
    blob = torch.randint(0, 256, (sum(lens),), dtype=torch.uint8,
                         generator=g).numpy().tobytes()
    rows, off = [], 0
    for ln in lens:
        rows.append(blob[off:off + ln])
        off += ln
    return rows


# -- bytes_gather ------------------------------------------------------------

def _check_gather(col, idx):
    idx = idx.to(DEV)
    want = col.select(idx)
    got = col.gather(idx)
    assert got.data.dtype == torch.uint8 and got.offsets.dtype == torch.int64
    assert torch.equal(got.offsets, want.offsets)
    assert torch.equal(got.data, want.data)
    # the byte count passed in, as the dictionary does
    total = int(want.data.shape[0])
    got = col.gather(idx, total=total)
    assert torch.equal(got.offsets, want.offsets)
    assert torch.equal(got.data, want.data)


def test_gather_empty_index_list(kernels):
    col = _column([b"ab", b"", b"cde"])
    _check_gather(col, torch.empty(0, dtype=torch.int64))


def test_gather_repeated_and_reversed(kernels):
    rows = _rand_rows(300, 0, 23, seed=1)
    col = _column(rows)
    n = len(rows)
    _check_gather(col, torch.arange(n - 1, -1, -1))
    _check_gather(col, torch.tensor([5, 5, 5, 0, 299, 5, 0, 299, 299]))
    g = torch.Generator().manual_seed(2)
    _check_gather(col, torch.randint(0, n, (1000,), generator=g))


def test_gather_all_rows_empty(kernels):
    col = _column([b""] * 50)
    _check_gather(col, torch.arange(50))
    mixed = _column([b"", b"abc", b""])
    _check_gather(mixed, torch.tensor([0, 2, 2, 0]))


@pytest.mark.parametrize("total", [15, 16, 17, 1, 31, 33, 4095, 4096, 4097])
def test_gather_totals_around_the_chunk(kernels, total):
    """One row per byte count, and the same bytes as rows of 1..5."""
    blob = bytes(range(256)) * 17
    col = _column([blob[:total], b"", blob[7:7 + total]])
    _check_gather(col, torch.tensor([0]))
    _check_gather(col, torch.tensor([1, 2, 1]))
    rows, off, k = [], 0, 0
    while off < total:
        ln = min(1 + k % 5, total - off)
        rows.append(blob[off:off + ln])
        off += ln
        k += 1
    small = _column(rows + [b""])
    idx = torch.arange(len(rows))
    want = small.select(idx.to(DEV))
    assert want.data.shape[0] == total
    _check_gather(small, idx)


def test_gather_one_long_row_among_short_ones(kernels):
    rows = _rand_rows(1000, 0, 9, seed=3)
    rows[417] = _rand_rows(1, 100_000, 100_000, seed=4)[0]
    col = _column(rows)
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 1000, (1000,), generator=g)
    idx[123] = 417
    idx[900] = 417
    _check_gather(col, idx)


def test_gather_from_a_slice_with_an_odd_base(kernels):
    rows = [b"abc"] + _rand_rows(500, 0, 30, seed=6)
    col = _column(rows)[1:400]
    assert int(col.offsets[0]) == 3
    g = torch.Generator().manual_seed(7)
    _check_gather(col, torch.randint(0, len(col), (700,), generator=g))
    _check_gather(col, torch.arange(len(col)))


def test_gather_more_than_one_workgroup(kernels):
    rows = _rand_rows(70_000, 0, 40, seed=8)
    col = _column(rows)
    g = torch.Generator().manual_seed(9)
    idx = torch.randint(0, 70_000, (70_000,), generator=g)
    want = col.select(idx.to(DEV))
    assert want.data.shape[0] > 4 * kernels._C.BYTES_GATHER_TILE_BYTES
    _check_gather(col, idx)


def test_gather_row_index_out_of_range_writes_nothing(kernels):
    col = _column([b"ab", b"cde", b"f"])
    idx = torch.tensor([1, 3, -1, 0, 1 << 40], dtype=torch.int64, device=DEV)
    got = col.gather(idx)
    assert got.offsets.tolist() == [0, 3, 3, 3, 5, 5]
    assert got.data.cpu().numpy().tobytes() == b"cdeab"


# -- IdDictionary --------------------------------------------------------------

def _check_dictionary(d, added, ndistinct):
    """added: [(column, ids)], all that went into d."""
    assert len(d) == ndistinct
    strings = d.strings()
    assert len(strings) == ndistinct
    words = strings.tolists()
    assert len(set(words)) == ndistinct
    for col, ids in added:
        pos = d.lookup(ids).cpu()
        if len(col) == 0:
            assert pos.numel() == 0
            continue
        assert int(pos.min()) >= 0 and int(pos.max()) < ndistinct
        assert [words[p] for p in pos.tolist()] == col.tolists()
    absent = torch.tensor([0x1234_5678_9ABC_DEF0, 3], dtype=torch.int64,
                          device=DEV)
    assert d.lookup(absent).tolist() == [-1, -1]


def _add(d, rows):
    col = _column(rows)
    ids = col.ids64() if rows else torch.empty(0, dtype=torch.int64,
                                               device=DEV)
    d.add(ids, col)
    return col, ids


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_dictionary_all_distinct(kernels, n):
    rows = [b"w%d" % i for i in range(n)]
    d = kernels.IdDictionary(DEV)
    added = [_add(d, rows)]
    _check_dictionary(d, added, n)
    # a batch added twice adds nothing
    added.append(_add(d, rows))
    _check_dictionary(d, added, n)


def test_dictionary_one_string_many_rows(kernels):
    d = kernels.IdDictionary(DEV)
    added = [_add(d, [b"the"] * 10_000)]
    _check_dictionary(d, added, 1)
    assert d.strings().tolists() == [b"the"]


def test_dictionary_overflow_regrows_and_claims_again(kernels):
    g = torch.Generator().manual_seed(11)
    vocab = [b"word-%d" % i for i in range(5000)]
    vocab[0] = b""
    d = kernels.IdDictionary(DEV, cap_hint=16)
    added, seen = [], set()
    for n in (30_000, 25_000, 15_000):
        idx = torch.randint(0, 5000, (n,), generator=g).tolist()
        rows = [vocab[i] for i in idx]
        seen.update(rows)
        added.append(_add(d, rows))
        assert len(d) == len(seen)
    assert d.regrows > 0 and d.cap > 16
    assert 2 * len(d) <= d.cap
    _check_dictionary(d, added, len(seen))


def test_dictionary_many_distinct_strings(kernels):
    rows = [b"k%07d" % (i * 7919) for i in range(100_000)]
    d = kernels.IdDictionary(DEV)
    added = [_add(d, rows)]
    _check_dictionary(d, added, 100_000)


def test_dictionary_empty_marker_is_id_zero(kernels):
    from bigslice_amd.kernels.groupby import GB_SENTINEL
    col = _column([b"same", b"same", b"other", b"same"])
    ids = torch.tensor([GB_SENTINEL, 0, 7, GB_SENTINEL], dtype=torch.int64,
                       device=DEV)
    d = kernels.IdDictionary(DEV)
    d.add(ids, col)
    assert len(d) == 2
    pos = d.lookup(ids).tolist()
    assert pos[0] == pos[1] == pos[3] != pos[2]
    words = d.strings().tolists()
    assert [words[p] for p in pos] == col.tolists()
    assert d.lookup(torch.tensor([1], device=DEV)).tolist() == [-1]


def test_dictionary_empty_batch(kernels):
    d = kernels.IdDictionary(DEV)
    added = [_add(d, [])]
    _check_dictionary(d, added, 0)
    added.append(_add(d, [b"a", b"b", b"a"]))
    added.append(_add(d, []))
    _check_dictionary(d, added, 2)
