"""Byte-order ranks of a BYTES column on the device (K24): the two HIP
kernels bit-equal to their CPU mirror, BytesColumn.order_ranks/argsort
equal to the CPU results, and Cogroup over keys with BYTES columns end
to end against a CPU session — key order unnormalised, since the order
is the point."""

import random

import pytest
import torch

from tests.test_bytesort import nasty_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BYTES = "bytes"


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    monkeypatch.delenv("BIGSLICE_COGROUP_BYTES", raising=False)


@pytest.fixture(scope="module")
def rows():
    return nasty_rows()


@pytest.fixture(scope="module")
def cols(rows):
    """(CPU column, device column)."""
    from bigslice_amd.frame import BytesColumn
    return BytesColumn.from_list(rows), BytesColumn.from_list(rows, DEV)


def _stat(name):
    from bigslice_amd.utils import stats
    return stats.DEFAULT.values().get(name, 0)


def _sizes(kernels):
    from bigslice_amd.kernels import bytesort
    return [1, 63, 64, 65, bytesort.KEYS_BLOCK + 1,
            bytesort.REFINE_TILE_SLOTS + 1]


# -- the kernels against the CPU mirror ----------------------------------------

@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "slice"])
def test_round_keys_bit_equal(kernels, cols, sliced):
    from bigslice_amd.kernels import bytesort
    cpu, dev = (c[5:-5] if sliced else c for c in cols)
    n = len(cpu)
    g = torch.Generator().manual_seed(3)
    for m in _sizes(kernels) + [n + 4]:
        if m <= n:
            idx = torch.randperm(n, generator=g)[:m]
            idx[-1] = n - 1  # the row at the end of the column
        else:
            idx = torch.cat([torch.arange(n),
                             torch.tensor([-1, n, n + 9, -n])])
        for w in range(7):
            want = bytesort.round_keys(cpu, idx, w)
            got = kernels._C.bytes_order_keys(
                dev.data, dev.offsets.contiguous(), idx.to(DEV), w)
            assert got.dtype == torch.int64 and got.is_cuda
            assert torch.equal(got.cpu(), want), (m, w)


def test_round_keys_on_an_unaligned_data_view(kernels, cols):
    """data that does not start on an 8-byte boundary, rows that end at
    its last byte: the byte-wise edge words."""
    from bigslice_amd.frame import BytesColumn
    from bigslice_amd.kernels import bytesort
    cpu, dev = cols
    for lead in (1, 3, 8, 13):
        start = int(cpu.offsets[lead])
        c = BytesColumn(cpu.data[start:], cpu.offsets[lead:] - start)
        d = BytesColumn(dev.data[start:], (dev.offsets[lead:] - start))
        idx = torch.arange(len(c))
        for w in (0, 1, 5):
            got = kernels._C.bytes_order_keys(
                d.data, d.offsets.contiguous(), idx.to(DEV), w)
            assert torch.equal(got.cpu(), bytesort.round_keys(c, idx, w))


def _sorted_slots(cpu, m, w, seed):
    """m slots as a round leaves them: sorted by (grp, key), with ties."""
    from bigslice_amd.kernels import bytesort
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, len(cpu), (m,), generator=g)
    key = bytesort.round_keys(cpu, idx, w)
    grp = torch.randint(0, max(1, m // 50), (m,), generator=g) * 50
    o = torch.sort(key, stable=True).indices
    o = o[torch.sort(grp[o], stable=True).indices]
    return grp[o].contiguous(), key[o].contiguous()


def test_refine_flags_bit_equal(kernels, cols):
    from bigslice_amd.kernels import bytesort
    cpu, _ = cols
    tile = bytesort.REFINE_TILE_SLOTS
    for m in _sizes(kernels) + [2, 3, 4, 5, tile - 1, tile, 2 * tile + 3]:
        for w in range(7):
            grp, key = _sorted_slots(cpu, m, w, m + w)
            want_head, want_stay = bytesort.refine(grp, key)
            head, stay = kernels._C.bytes_order_refine(grp.to(DEV),
                                                       key.to(DEV))
            assert stay.dtype == torch.bool
            assert torch.equal(head.cpu(), want_head), (m, w)
            assert torch.equal(stay.cpu(), want_stay), (m, w)


def test_kernels_at_70k_rows(kernels, cols):
    """The key kernel's grid-stride loop (a grid of 64 workgroups takes
    16384 rows a pass) and 69 tiles of the refine kernel with ties
    across their edges."""
    from bigslice_amd.kernels import bytesort
    cpu, dev = cols
    m = 70_001
    g = torch.Generator().manual_seed(70)
    idx = torch.randint(-2, len(cpu) + 2, (m,), generator=g)
    for w in (0, 1, 2):
        want = bytesort.round_keys(cpu, idx, w)
        for max_blocks in (0, 64):
            got = kernels._C.bytes_order_keys(dev.data, dev.offsets,
                                              idx.to(DEV), w, max_blocks)
            assert torch.equal(got.cpu(), want)
        grp, key = _sorted_slots(cpu, m, w, 71 + w)
        want_head, want_stay = bytesort.refine(grp, key)
        assert want_stay.any() and not want_stay.all()
        head, stay = kernels._C.bytes_order_refine(grp.to(DEV),
                                                   key.to(DEV))
        assert torch.equal(head.cpu(), want_head)
        assert torch.equal(stay.cpu(), want_stay)


# -- ranks ---------------------------------------------------------------------

def test_order_ranks_and_argsort_equal_the_cpu_results(kernels, cols, rows):
    cpu, dev = cols
    ranks = dev.order_ranks()
    assert ranks.is_cuda and ranks.dtype == torch.int64
    assert torch.equal(ranks.cpu(), cpu.order_ranks())
    perm = dev.argsort()
    assert torch.equal(perm.cpu(), cpu.argsort())
    assert perm.cpu().tolist() == sorted(range(len(rows)),
                                         key=lambda i: rows[i])
    part = dev[5:-5]
    assert torch.equal(part.order_ranks().cpu(), cpu[5:-5].order_ranks())
    assert torch.equal(part.argsort().cpu(), cpu[5:-5].argsort())


def test_distinct_ranks_and_rounds_equal_the_cpu_results(kernels, rows):
    from bigslice_amd.frame import BytesColumn
    from bigslice_amd.kernels import bytesort
    distinct = sorted(set(rows), key=lambda r: (len(r), r))
    on_cpu, on_dev = {}, {}
    want = bytesort.distinct_order_ranks(BytesColumn.from_list(distinct),
                                         on_cpu)
    got = bytesort.distinct_order_ranks(
        BytesColumn.from_list(distinct, DEV), on_dev)
    assert torch.equal(got.cpu(), want)
    assert on_dev == on_cpu and on_cpu["rounds"] >= 6


# -- Cogroup end to end --------------------------------------------------------

_WORDS = {}


def _words(rows):
    """About 300 words, the nasty strings among them."""
    if not _WORDS:
        distinct = sorted(set(rows))
        nasty = [r for r in distinct if len(r) > 20 or r in (
            b"", b"a", b"a\0", b"a\0\0", b"\x7f", b"\x80", b"\xff",
            b"1234567", b"12345678", b"fourteen-bytes",
            b"fourteen-bytes!", b"fourteen-bytes\0")]
        _WORDS["w"] = nasty + [r for r in distinct[::9] if r not in nasty]
    return _WORDS["w"]


def _side(n, key_dts, words, seed, val_dtypes=(torch.int64,), hi=3):
    from bigslice_amd.frame import BytesColumn
    rng = random.Random(seed)
    cols = []
    for dt in key_dts:
        if dt == BYTES:
            cols.append(BytesColumn.from_list(
                [rng.choice(words) for _ in range(n)]))
        else:
            cols.append(torch.tensor(
                [rng.randrange(-hi, hi) for _ in range(n)], dtype=dt))
    g = torch.Generator().manual_seed(seed)
    for dt in val_dtypes:
        cols.append(torch.randint(-10**6, 10**6, (n,), dtype=torch.int64,
                                  generator=g).to(dt))
    return cols


def _run(sides, nkey, device, frames_out=None):
    import bigslice_amd as bs

    def job():
        return bs.Cogroup(*[bs.Prefixed(bs.Const(3, *cols), nkey)
                            for cols in sides])
    sess = bs.start(parallelism=2, device=device)
    res = sess.run(bs.func(job))
    frames = [f for f in res.open() if len(f)]
    if frames_out is not None:
        frames_out.extend(frames)
    out = [[r for r in f.rows()] for f in frames]
    sess.shutdown()
    return out


def _same_on_device(sides, nkey, frames_out=None):
    """Per output frame (the shards come back in shard order): the keys
    in the order they come, the value lists as sorted multisets."""
    want = _run(sides, nkey, "cpu")
    before = _stat("cogroup/bytes_device")
    got = _run(sides, nkey, DEV, frames_out)
    assert _stat("cogroup/bytes_device") > before
    flat_want = [r for f in want for r in f]
    flat_got = [r for f in got for r in f]
    assert len(flat_want) > 0
    assert ([tuple(r[:nkey]) for r in flat_got]
            == [tuple(r[:nkey]) for r in flat_want])
    assert ([tuple(tuple(sorted(v)) for v in r[nkey:]) for r in flat_got]
            == [tuple(tuple(sorted(v)) for v in r[nkey:])
                for r in flat_want])
    return flat_want


def test_cogroup_one_bytes_key_two_deps(kernels, rows):
    from bigslice_amd.frame import BytesColumn, SegmentedColumn
    words = _words(rows)
    assert 250 <= len(words) <= 350
    sides = [_side(4000, [BYTES], words, 1), _side(3000, [BYTES], words, 2)]
    frames = []
    got = _same_on_device(sides, 1, frames)
    assert len(got) == len(words)
    # the frames the GPU reader emits stay on the device
    assert frames
    for f in frames:
        assert isinstance(f.columns[0], BytesColumn)
        assert f.columns[0].data.is_cuda
        for c in f.columns[1:]:
            assert isinstance(c, SegmentedColumn) and c.values.is_cuda
        keys = f.columns[0].tolists()
        assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.mark.parametrize("key_dts", [[BYTES, torch.int64],
                                     [torch.int32, BYTES]], ids=str)
def test_cogroup_composite_keys(kernels, rows, key_dts):
    words = _words(rows)[:60]
    sides = [_side(4000, key_dts, words, 3), _side(3000, key_dts, words, 4)]
    _same_on_device(sides, 2)


def test_cogroup_three_deps(kernels, rows):
    words = _words(rows)
    sides = [_side(2000, [BYTES], words, 5), _side(1500, [BYTES], words, 6),
             _side(1000, [BYTES], words[::3], 7)]
    _same_on_device(sides, 1)


def test_cogroup_keys_present_in_only_one_side(kernels, rows):
    words = _words(rows)
    a = _side(1500, [BYTES], words[::2], 8)
    b = _side(1500, [BYTES], words[1::2], 9)
    got = _same_on_device([a, b], 1)
    assert all((len(r[1]) == 0) != (len(r[2]) == 0) for r in got)
    # and a partial overlap
    b = _side(1500, [BYTES], words[1::2] + words[::4], 10)
    got = _same_on_device([a, b], 1)
    assert any(len(r[1]) and len(r[2]) for r in got)
    assert any(len(r[1]) == 0 or len(r[2]) == 0 for r in got)


def test_cogroup_one_empty_side(kernels, rows):
    words = _words(rows)
    a = _side(2000, [BYTES, torch.int64], words[:40], 11)
    b = [c[:0] for c in _side(4, [BYTES, torch.int64], words[:40], 12)]
    got = _same_on_device([a, b], 2)
    assert all(len(r[3]) == 0 for r in got)
    got = _same_on_device([b, a], 2)
    assert all(len(r[2]) == 0 for r in got)


def test_cogroup_two_value_columns_of_different_dtypes(kernels, rows):
    words = _words(rows)
    a = _side(2000, [BYTES], words, 13,
              val_dtypes=(torch.int64, torch.float32))
    b = _side(1500, [BYTES], words, 14, val_dtypes=(torch.int32,))
    _same_on_device([a, b], 1)


def test_cogroup_switch_off_gives_the_same_rows(kernels, rows, monkeypatch):
    words = _words(rows)
    sides = [_side(3000, [BYTES, torch.int64], words[:80], 15),
             _side(2000, [BYTES, torch.int64], words[:80], 16)]
    want = _same_on_device(sides, 2)
    ran = _stat("cogroup/bytes_device")
    monkeypatch.setenv("BIGSLICE_COGROUP_BYTES", "0")
    got = [r for f in _run(sides, 2, DEV) for r in f]
    assert _stat("cogroup/bytes_device") == ran
    assert [tuple(r[:2]) for r in got] == [tuple(r[:2]) for r in want]
    assert ([tuple(tuple(sorted(v)) for v in r[2:]) for r in got]
            == [tuple(tuple(sorted(v)) for v in r[2:]) for r in want])
