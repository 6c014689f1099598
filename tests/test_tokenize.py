"""BytesColumn.split / from_buffer, the Tokenize operator, vectorized
UDFs returning a BytesColumn, and recipes.device_wordcount, all on the
host path.  The oracle is Python itself: bytes.split() for the default
delimiter set, re.split for custom sets, collections.Counter for counts."""

import random
import re
from collections import Counter

import pytest
import torch

import bigslice_amd as bs
from bigslice_amd import recipes
from bigslice_amd.frame import BytesColumn
from bigslice_amd.schema import BYTES, OBJECT, Schema


def oracle(rows, delims=None):
    """(tokens, source row of each token)."""
    toks, src = [], []
    for i, row in enumerate(rows):
        if delims is None:
            parts = row.split()
        else:
            cls = b"[" + b"".join(re.escape(bytes([d])) for d in delims) \
                + b"]+"
            parts = [t for t in re.split(cls, row) if t]
        toks.extend(parts)
        src.extend([i] * len(parts))
    return toks, src


def check(rows, delims=None, col=None):
    col = BytesColumn.from_list(rows) if col is None else col
    want, want_rows = oracle(rows, delims)
    got = col.split(delims)
    assert isinstance(got, BytesColumn)
    assert got.tolists() == want
    got2, rws = col.split(delims, with_rows=True)
    assert got2.tolists() == want
    assert rws.dtype == torch.int64 and rws.tolist() == want_rows
    # zero-based contiguous offsets over exactly the kept bytes
    assert got.offsets.dtype == torch.int64 and got.data.dtype == torch.uint8
    assert int(got.offsets[0]) == 0
    assert int(got.offsets[-1]) == got.data.numel() == sum(map(len, want))
    assert torch.equal(got.data, got2.data)
    assert torch.equal(got.offsets, got2.offsets)
    return got


HAND = [
    [],
    [b""],
    [b"", b"", b"a b", b"", b"c", b"", b""],
    [b"   ", b"\t\n", b"x", b" \r\x0b\x0c "],
    [b"nodelimiter"],
    [b"  lead", b"trail  ", b"a   b\t\tc", b" \n x \n "],
    [b"ab", b"cd"],
    [b"\x00\x80\xff", b"a\x00b \x80 \xff\xff"],
]


@pytest.mark.parametrize("rows", HAND)
def test_split_hand_made(rows):
    check(rows)


def test_split_adjacent_rows_are_two_tokens():
    got = check([b"ab", b"cd"])
    assert got.tolists() == [b"ab", b"cd"]


def test_split_custom_set_with_00_and_ff():
    rows = [b"a\x00b\xffc", b"\x00\x00", b" x \xff y\x80", b"", b"\xffz\x00"]
    got = check(rows, b"\x00\xff")
    assert got.tolists() == [b"a", b"b", b"c", b" x ", b" y\x80", b"z"]
    check(rows, b",")
    check([b"a,b;;c", b";", b"d"], b",;")


def test_split_rejects_empty_set():
    col = BytesColumn.from_list([b"a b"])
    with pytest.raises(ValueError):
        col.split(b"")


def test_split_with_rows_indices():
    col = BytesColumn.from_list([b"", b"a b", b"  ", b"c", b"d e f"])
    toks, rows = col.split(with_rows=True)
    assert toks.tolists() == [b"a", b"b", b"c", b"d", b"e", b"f"]
    assert rows.tolist() == [1, 1, 3, 4, 4, 4]


def test_split_zero_copy_slice():
    rng = random.Random(5)
    rows = [bytes(rng.choice(b"ab \t") for _ in range(rng.randrange(0, 9)))
            for _ in range(20)]
    col = BytesColumn.from_list(rows)
    sl = col[3:17]
    assert int(sl.offsets[0]) > 0  # still absolute into the parent
    check(rows[3:17], col=sl)
    check(rows[3:17], b"a", col=sl)


def test_from_buffer_multi_line_chunk():
    text = b"the quick\nbrown  fox\n\njumps\tover\r\nthe lazy dog\n"
    col = BytesColumn.from_buffer(text)
    assert len(col) == 1 and col.tolists() == [text]
    toks, rows = col.split(with_rows=True)
    assert toks.tolists() == text.split()
    assert rows.tolist() == [0] * len(text.split())
    assert BytesColumn.from_buffer(bytearray(b"a b")).split().tolists() \
        == [b"a", b"b"]
    assert BytesColumn.from_buffer(b"").split().tolists() == []


def test_split_seeded_random_columns():
    rng = random.Random(1234)
    alphabet = b"abc \t\n"
    for _ in range(300):
        rows = [bytes(rng.choice(alphabet)
                      for _ in range(rng.randrange(0, 41)))
                for _ in range(rng.randrange(0, 12))]
        check(rows)
    for _ in range(50):
        rows = [bytes(rng.choice(alphabet)
                      for _ in range(rng.randrange(0, 41)))
                for _ in range(rng.randrange(0, 12))]
        check(rows, b"a\n")


# -- Tokenize on a CPU session ------------------------------------------------

@pytest.fixture(scope="module")
def sess():
    return bs.start(parallelism=2, device="cpu")


def run(sess, build, *args):
    res = sess.run(bs.func(build), *args)
    rows = list(res.scan())
    res.discard()
    return rows


LINES = ["the cat  sat", "", "on the\tmat", "   ", "the end"] * 7


def test_tokenize_bytes_input(sess):
    enc = [ln.encode() for ln in LINES]

    def build(nshard):
        def gen(shard, ctx):
            yield (BytesColumn.from_list(enc[shard::nshard]),)
        return bs.Tokenize(bs.ReaderFunc(nshard, gen, bs.schema_of(bytes)))
    got = run(sess, build, 2)
    assert Counter(got) == Counter(w for ln in enc for w in ln.split())


def test_tokenize_object_input(sess):
    def build(nshard):
        return bs.Tokenize(bs.ScanReader(nshard, lambda: iter(LINES)))
    got = run(sess, build, 3)
    assert Counter(got) == Counter(w.encode() for ln in LINES
                                   for w in ln.split())


def test_tokenize_custom_delims(sess):
    def build(nshard):
        return bs.Tokenize(bs.ScanReader(nshard, lambda: iter(LINES)),
                           delims=b"te")
    got = run(sess, build, 1)
    want = [t for ln in LINES for t in re.split(b"[te]+", ln.encode()) if t]
    assert got == want


def test_tokenize_carried_columns_repeat_per_token(sess):
    enc = [ln.encode() for ln in LINES]
    tags = [b"tag%d" % (i % 4) for i in range(len(enc))]

    def build(nshard):
        def gen(shard, ctx):
            idx = list(range(shard, len(enc), nshard))
            yield (BytesColumn.from_list([enc[i] for i in idx]),
                   torch.tensor(idx, dtype=torch.int64),
                   BytesColumn.from_list([tags[i] for i in idx]))
        src = bs.ReaderFunc(nshard, gen, bs.schema_of(bytes, int, bytes))
        return bs.Tokenize(src)
    got = run(sess, build, 2)
    want = [(w, i, tags[i]) for i, ln in enumerate(enc) for w in ln.split()]
    assert sorted(got) == sorted(want)


def test_tokenize_carried_object_column_and_col1(sess):
    enc = [ln.encode() for ln in LINES]

    def build(nshard):
        def gen(shard, ctx):
            idx = list(range(shard, len(enc), nshard))
            yield ([f"id{i}" for i in idx],
                   BytesColumn.from_list([enc[i] for i in idx]))
        src = bs.ReaderFunc(nshard, gen, bs.schema_of(str, bytes))
        return bs.Tokenize(src, col=1)
    got = run(sess, build, 2)
    want = [(f"id{i}", w) for i, ln in enumerate(enc) for w in ln.split()]
    assert sorted(got) == sorted(want)


def test_tokenize_schema_and_prefix():
    src = bs.Const(1, ["a b"], [1], [2.0])
    assert src.schema == Schema([OBJECT, torch.int64, torch.float64], 1)
    tok = bs.Tokenize(src)
    assert tok.schema == Schema([BYTES, torch.int64, torch.float64], 1)
    assert bs.Tokenize(src, prefix=2).schema.prefix == 2
    assert "tokenize" in str(tok.name)
    with pytest.raises(TypeError):
        bs.Tokenize(src, col=1)
    with pytest.raises(TypeError):
        bs.Tokenize(src, col=3)
    with pytest.raises(ValueError):
        bs.Tokenize(src, delims=b"")


# -- vectorized UDFs returning a BytesColumn ----------------------------------

def test_map_returning_bytescolumn(sess):
    def build(nshard):
        words = bs.Tokenize(bs.ScanReader(nshard, lambda: iter(LINES)))
        return bs.Map(
            words,
            lambda w: (w, torch.ones(len(w), dtype=torch.int64,
                                     device=w.device)),
            out_schema=(bytes, int))
    got = run(sess, build, 2)
    want = [(w.encode(), 1) for ln in LINES for w in ln.split()]
    assert sorted(got) == sorted(want)


def test_flatmap_returning_bytescolumn(sess):
    enc = [ln.encode() for ln in LINES]

    def build(nshard):
        def gen(shard, ctx):
            yield (BytesColumn.from_list(enc[shard::nshard]),)
        src = bs.ReaderFunc(nshard, gen, bs.schema_of(bytes))
        return bs.Flatmap(src, lambda c: (c.split(),), out_schema=(bytes,))
    got = run(sess, build, 2)
    assert Counter(got) == Counter(w for ln in enc for w in ln.split())


# -- the recipe ------------------------------------------------------------

@pytest.mark.parametrize("nshard", [1, 3])
def test_device_wordcount_cpu_session(sess, nshard):
    rng = random.Random(nshard)
    vocab = [f"w{i}" for i in range(50)]
    lines = [" ".join(rng.choice(vocab) for _ in range(rng.randrange(0, 9)))
             for _ in range(200)]
    ref = Counter(w for ln in lines for w in ln.split())

    def build(n):
        return recipes.device_wordcount(n, lambda: iter(lines))
    got = run(sess, build, nshard)
    assert len(got) == len(ref)
    assert {k.decode(): v for k, v in got} == dict(ref)
