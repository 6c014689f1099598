"""Multi-column group-by keys (K21), the part that needs no device: the
torch mirror of the tuple fingerprint, against a plain-Python-integer
implementation written here, and the CPU routing of make_aggregator."""

import itertools

import pytest
import torch

from bigslice_amd.kernels.groupby_multi import (GB_HASH_SEED, Options,
                                                fingerprint64)

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1
M64 = (1 << 64) - 1

EDGE = [0, -1, INT64_MIN, INT64_MAX, 1, 2, -2, 0x9ACB0442, 1 << 32,
        -(1 << 32), 1234567890123456789]


def _fmix64(h):
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return h


def _py_fingerprint(tup, fp_bits=64):
    """The tag of one tuple of Python integers, on unsigned 64-bit
    arithmetic; returned as the signed value of the same bits."""
    h = GB_HASH_SEED
    for k in tup:
        h = _fmix64(((h + 0x9E3779B97F4A7C15) & M64) ^ (k & M64))
    h &= (1 << fp_bits) - 1
    if h == 1 << 63:  # the bits of the empty marker
        h = 0
    return h - (1 << 64) if h >> 63 else h


def _cols(tuples):
    return [torch.tensor(list(c), dtype=torch.int64) for c in zip(*tuples)]


@pytest.mark.parametrize("ncols", [2, 3, 8])
def test_matches_python_integers(ncols):
    g = torch.Generator().manual_seed(ncols)
    tuples = [tuple(EDGE[(i + 3 * c) % len(EDGE)] for c in range(ncols))
              for i in range(len(EDGE))]
    tuples += list(itertools.product([0, -1, INT64_MIN, INT64_MAX],
                                     repeat=2))[:16] if ncols == 2 else []
    rnd = torch.randint(INT64_MIN, INT64_MAX, (200, ncols),
                        dtype=torch.int64, generator=g)
    tuples += [tuple(r) for r in rnd.tolist()]
    got = fingerprint64(_cols(tuples)).tolist()
    assert got == [_py_fingerprint(t) for t in tuples]


def test_order_sensitive():
    a = torch.tensor([1, 7, -5, INT64_MIN, 0, 123456789], dtype=torch.int64)
    b = torch.tensor([2, 9, 5, INT64_MAX, -1, 987654321], dtype=torch.int64)
    ab, ba = fingerprint64([a, b]), fingerprint64([b, a])
    assert not (ab == ba).any()
    aa, bb = fingerprint64([a, a]), fingerprint64([b, b])
    assert not (aa == bb).any()
    # the positions of three columns, too
    c = a + 100
    prints = {tuple(fingerprint64(list(p)).tolist())
              for p in itertools.permutations([a, b, c])}
    assert len(prints) == 6


def _preimage(target, ncols):
    """A tuple whose unmasked hash is `target`: the chain is made of
    bijections, so its last column can be solved for."""
    def unshift(h):  # inverse of h ^= h >> 33
        return h ^ (h >> 33)

    def unfmix(h):
        h = unshift(h)
        h = (h * pow(0xC4CEB9FE1A85EC53, -1, 1 << 64)) & M64
        h = unshift(h)
        h = (h * pow(0xFF51AFD7ED558CCD, -1, 1 << 64)) & M64
        return unshift(h)
    head = list(range(5, 5 + ncols - 1))
    h = GB_HASH_SEED
    for k in head:
        h = _fmix64(((h + 0x9E3779B97F4A7C15) & M64) ^ k)
    last = unfmix(target) ^ ((h + 0x9E3779B97F4A7C15) & M64)
    last = last - (1 << 64) if last >> 63 else last
    return tuple(head) + (last,)


@pytest.mark.parametrize("ncols", [2, 3])
def test_never_the_sentinel(ncols):
    # a tuple that hashes to the empty marker's bits gets tag 0 ...
    tup = _preimage(1 << 63, ncols)
    assert _py_fingerprint(tup) == 0
    assert fingerprint64(_cols([tup])).tolist() == [0]
    # ... and its neighbour keeps its own hash
    near = _preimage((1 << 63) + 1, ncols)
    assert fingerprint64(_cols([near])).tolist() == [INT64_MIN + 1]
    g = torch.Generator().manual_seed(1)
    cols = [torch.randint(INT64_MIN, INT64_MAX, (100_000,),
                          dtype=torch.int64, generator=g)
            for _ in range(ncols)]
    for bits in (64, 63, 8):
        assert not (fingerprint64(cols, bits) == INT64_MIN).any()


@pytest.mark.parametrize("bits", [1, 4, 31, 32, 33, 63])
def test_honours_fp_bits(bits):
    g = torch.Generator().manual_seed(bits)
    cols = [torch.randint(INT64_MIN, INT64_MAX, (4096,), dtype=torch.int64,
                          generator=g) for _ in range(2)]
    full = fingerprint64(cols)
    masked = fingerprint64(cols, bits)
    assert torch.equal(masked, full & ((1 << bits) - 1))
    assert int(masked.min()) >= 0 and int(masked.max()) < (1 << bits)
    assert masked.tolist()[:64] == [
        _py_fingerprint(t, bits)
        for t in zip(cols[0].tolist()[:64], cols[1].tolist()[:64])]
    if bits <= 4:
        assert len(set(masked.tolist())) == 1 << bits
    with pytest.raises(ValueError):
        fingerprint64(cols, 0)
    with pytest.raises(ValueError):
        fingerprint64(cols, 65)


def test_options_read_the_environment():
    assert Options.from_env({}) == Options(enabled=True, fp_bits=64)
    o = Options.from_env({"BIGSLICE_GB_MULTIKEY": "0",
                          "BIGSLICE_GB_FP_BITS": "4"})
    assert o == Options(enabled=False, fp_bits=4)
    with pytest.raises(ValueError):
        Options.from_env({"BIGSLICE_GB_FP_BITS": "65"})


def test_eligible_shapes():
    from bigslice_amd.kernels.groupby_multi import multikey_supported
    i64, i32, f32 = torch.int64, torch.int32, torch.float32
    assert multikey_supported([i64, i32], [i64, f32], ["sum", "max"])
    assert multikey_supported([i64] * 8, [i64] * 8, ["sum"] * 8)
    assert not multikey_supported([i64] * 8, [i64] * 9, ["sum"] * 9)
    assert not multikey_supported([i64] * 9, [i64], ["sum"])
    assert not multikey_supported([i64], [i64], ["sum"])
    assert not multikey_supported([i64, f32], [i64], ["sum"])
    assert not multikey_supported([i64, i64], [torch.int8], ["sum"])
    assert not multikey_supported([i64, i64], [i64], [max])


def test_cpu_aggregator_has_no_table():
    from bigslice_amd.frame import Frame
    from bigslice_amd.ops.aggregate import (Aggregation, TensorAggregator,
                                            make_aggregator)
    from bigslice_amd.schema import Schema
    schema = Schema((torch.int64, torch.int64, torch.int64), 2)
    agg = make_aggregator(schema, Aggregation(["sum"]), "cpu")
    assert isinstance(agg, TensorAggregator) and agg._table is None
    k1 = torch.tensor([1, 2, 1, 2, 1], dtype=torch.int64)
    k2 = torch.tensor([5, 5, 6, 5, 5], dtype=torch.int64)
    v = torch.tensor([1, 10, 100, 1000, 10000], dtype=torch.int64)
    agg.add(Frame([k1, k2, v], 2))
    rows = sorted(tuple(int(c[i]) for c in f.columns)
                  for f in agg.result_frames(1 << 20)
                  for i in range(len(f)))
    assert rows == [(1, 5, 10001), (1, 6, 100), (2, 5, 1010)]
