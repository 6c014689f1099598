"""The tokenizer kernels (csrc/tokenize.hip) through kernels.tokenize_bytes:
data, offsets and rows bit for bit against Python's own split and against
the host path, at every size and placement where a tile edge, a wave edge
or a row edge can go wrong; then Tokenize and device_wordcount on a GPU
session against a CPU session."""

import random
import re
from collections import Counter

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALPHABET = np.frombuffer(b"abc \t\n", dtype=np.uint8)


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


def random_text(rng, total, alphabet=ALPHABET):
    return alphabet[rng.integers(0, len(alphabet), total)].tobytes()


def random_cuts(rng, total, nrows):
    """Sorted row boundaries [0, ..., total]; repeats are empty rows."""
    inner = np.sort(rng.integers(0, total + 1, max(nrows - 1, 0)))
    return [0] + inner.tolist() + [total]


def column(buf, cuts, device="cpu"):
    from bigslice_amd.frame import BytesColumn
    data = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy())
    return BytesColumn(data.to(device),
                       torch.tensor(cuts, dtype=torch.int64).to(device))


def oracle(buf, cuts, delims=None):
    """Python's split per row, as the three expected tensors."""
    toks, src = [], []
    pat = None if delims is None else re.compile(
        b"[" + b"".join(re.escape(bytes([d])) for d in delims) + b"]+")
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        row = buf[a:b]
        parts = row.split() if pat is None else \
            [t for t in pat.split(row) if t]
        toks.extend(parts)
        src.extend([i] * len(parts))
    offs = np.zeros(len(toks) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in toks], out=offs[1:])
    data = np.frombuffer(b"".join(toks), dtype=np.uint8).copy()
    return (torch.from_numpy(data), torch.from_numpy(offs),
            torch.tensor(src, dtype=torch.int64))


def check(kernels, buf, cuts, delims=None, col=None):
    """Native wrapper (never the dispatching split(), so a fallback
    cannot pass) against the oracle and against the host path."""
    from bigslice_amd.frame import split_torch
    gcol = (column(buf, cuts, DEV) if col is None else col).compacted()
    assert gcol.data.is_cuda
    mask4 = kernels.tokenize_mask(delims)
    got = kernels.tokenize_bytes(gcol.data, gcol.offsets, mask4, True)
    got2 = kernels.tokenize_bytes(gcol.data, gcol.offsets, mask4, False)
    assert len(got) == 3 and len(got2) == 2
    want = oracle(buf, cuts, delims)
    host = split_torch(gcol.data.cpu(), gcol.offsets.cpu(), mask4, True)
    for name, g, w, h in zip(("data", "offsets", "rows"), got, want, host):
        g = g.cpu()
        assert g.dtype == w.dtype == h.dtype, name
        assert torch.equal(g, w), f"{name} differs from Python's split"
        assert torch.equal(g, h), f"{name} differs from the host path"
    assert torch.equal(got2[0], got[0]) and torch.equal(got2[1], got[1])
    return got


SIZES = ["0", "1", "15", "16", "17", "63", "64", "65",
         "T-1", "T", "T+1", "2*T+3", "70*T+5"]


@pytest.mark.parametrize("size", SIZES)
def test_sizes(kernels, size):
    T = kernels.TOKENIZE_TILE_BYTES
    total = eval(size, {"T": T})
    rng = np.random.default_rng(total + 7)
    buf = random_text(rng, total)
    cuts = random_cuts(rng, total, max(1, total // 20)) if total else [0]
    check(kernels, buf, cuts)
    if total:
        check(kernels, buf, [0, total])
    else:
        check(kernels, buf, [0, 0, 0])  # rows without bytes


def _placed(T):
    rng = np.random.default_rng(99)

    def text(n):
        return bytearray(random_text(rng, n))
    cases = {}
    b = text(2 * T + 100)
    b[T - 5:T + 5] = b"abcabcabca"
    cases["token across a tile edge"] = (b, [0, len(b)])
    b = text(5 * T)
    b[T - 2:4 * T + 2] = b"a" * (3 * T + 4)
    cases["token covering three tiles"] = (b, [0, 7, len(b)])
    b = text(3 * T)
    b[T:2 * T] = b" " * T
    cases["tile of delimiters"] = (b, random_cuts(rng, len(b), 40))
    b = text(2 * T)
    b[T - 1:T + 1] = b"ab"
    cases["row edge at T between letters"] = (b, [0, T, 2 * T])
    b = text(2 * T)
    b[T - 1:T + 1] = b" a"
    cases["delimiter ends a tile"] = (b, [0, 5, 2 * T])
    b = text(2 * T + 9)
    b[T - 1:T + 1] = b"ab"
    cases["5000 empty rows at T"] = (b, [0] + [T] * 5001 + [len(b)])
    cases["5000 empty rows at 0"] = (b, [0] * 5001 + [len(b)])
    cases["5000 empty rows at total"] = (b, [0] + [len(b)] * 5001)
    return cases


PLACED = ["token across a tile edge", "token covering three tiles",
          "tile of delimiters", "row edge at T between letters",
          "delimiter ends a tile", "5000 empty rows at T",
          "5000 empty rows at 0", "5000 empty rows at total"]


@pytest.mark.parametrize("name", PLACED)
def test_placed(kernels, name):
    buf, cuts = _placed(kernels.TOKENIZE_TILE_BYTES)[name]
    check(kernels, bytes(buf), cuts)


def test_row_edge_at_tile_edge_splits_token(kernels):
    T = kernels.TOKENIZE_TILE_BYTES
    buf = b"a" * (2 * T)
    got = check(kernels, buf, [0, T, 2 * T])
    assert got[1].tolist() == [0, T, 2 * T] and got[2].tolist() == [0, 1]
    got = check(kernels, buf, [0, 2 * T])
    assert got[1].tolist() == [0, 2 * T]


def test_single_row_from_buffer(kernels):
    from bigslice_amd.frame import BytesColumn
    T = kernels.TOKENIZE_TILE_BYTES
    rng = np.random.default_rng(3)
    buf = random_text(rng, 3 * T + 7)
    col = BytesColumn.from_buffer(buf, DEV)
    assert len(col) == 1 and col.data.is_cuda
    check(kernels, buf, [0, len(buf)], col=col)
    toks = col.split()
    assert toks.data.is_cuda and toks.tolists() == buf.split()


def test_high_bytes_are_data(kernels):
    T = kernels.TOKENIZE_TILE_BYTES
    rng = np.random.default_rng(11)
    alphabet = np.array([0x00, 0x80, 0xFF, 0x41, 0x20, 0xFE, 0x7F],
                        dtype=np.uint8)
    buf = random_text(rng, 2 * T + 3, alphabet)
    cuts = random_cuts(rng, len(buf), 300)
    check(kernels, buf, cuts, delims=b"\x00\xff")
    check(kernels, buf, cuts)  # 0x80.. are plain data for whitespace too


def test_sliced_column(kernels):
    T = kernels.TOKENIZE_TILE_BYTES
    rng = np.random.default_rng(21)
    buf = random_text(rng, 3 * T + 11)
    cuts = random_cuts(rng, len(buf), 500)
    parent = column(buf, cuts, DEV)
    # first row of the slice starts mid-tile at an odd byte of the parent
    k = next(i for i in range(100, len(cuts)) if cuts[i] % 2 == 1)
    sl = parent[k:len(cuts) - 3]
    assert int(sl.offsets[0]) == cuts[k] and cuts[k] % T != 0
    sub = cuts[k:len(cuts) - 2]
    lo = sub[0]
    check(kernels, buf[lo:sub[-1]], [c - lo for c in sub], col=sl)
    toks, rows = sl.split(with_rows=True)
    want = oracle(buf[lo:sub[-1]], [c - lo for c in sub])
    assert torch.equal(toks.data.cpu(), want[0])
    assert torch.equal(rows.cpu(), want[2])


def test_split_dispatches_to_kernel_and_matches_cpu(kernels):
    rng = np.random.default_rng(5)
    buf = random_text(rng, 50_000)
    cuts = random_cuts(rng, len(buf), 2000)
    g, grows = column(buf, cuts, DEV).split(with_rows=True)
    c, crows = column(buf, cuts).split(with_rows=True)
    assert g.data.is_cuda and grows.is_cuda
    assert torch.equal(g.data.cpu(), c.data)
    assert torch.equal(g.offsets.cpu(), c.offsets)
    assert torch.equal(grows.cpu(), crows)


# -- through the engine ------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    rng = random.Random(17)
    vocab = [f"w{i:04d}" for i in range(2000)]
    return [" ".join(rng.choice(vocab) for _ in range(8))
            for _ in range(20_000)]


def _run(device, build, *args):
    import bigslice_amd as bs
    sess = bs.start(parallelism=4, device=device)
    res = sess.run(bs.func(build), *args)
    rows = list(res.scan())
    res.discard()
    return rows


def test_device_wordcount_gpu_session(kernels, corpus):
    from bigslice_amd import recipes
    ref = Counter(w for ln in corpus for w in ln.split())

    def build(nshard):
        return recipes.device_wordcount(nshard, lambda: iter(corpus))
    gpu = _run(DEV, build, 4)
    assert len(gpu) == len(ref)
    assert {k.decode(): v for k, v in gpu} == dict(ref)
    cpu = _run("cpu", build, 4)
    assert sorted(gpu) == sorted(cpu)


def test_tokenize_carried_column_gpu_session(kernels, corpus):
    import bigslice_amd as bs
    from bigslice_amd.frame import BytesColumn
    lines = [ln.encode() for ln in corpus[:3000]]

    def build(nshard):
        def gen(shard, ctx):
            idx = list(range(shard, len(lines), nshard))
            yield (BytesColumn.from_list([lines[i] for i in idx],
                                         ctx.device),
                   torch.tensor(idx, dtype=torch.int64, device=ctx.device))
        src = bs.ReaderFunc(nshard, gen, bs.schema_of(bytes, int))
        return bs.Tokenize(src)
    gpu = _run(DEV, build, 3)
    cpu = _run("cpu", build, 3)
    want = [(w, i) for i, ln in enumerate(lines) for w in ln.split()]
    assert sorted(gpu) == sorted(want)
    assert sorted(gpu) == sorted(cpu)
