"""Expression vocabulary (exprs.py) on the CPU: Expr.eval against
hand-written torch, the bytecode lowering against Expr.eval through the
host interpreter, construction errors, and Map/Filter chains written
with Exprs against the same chains written with lambdas."""

import random

import pytest
import torch

import bigslice_amd as bs
from bigslice_amd import exprs
from bigslice_amd.exprs import (ExprReader, compile_program,
                                run_program_host)
from bigslice_amd.schema import BYTES, OBJECT, Schema

I64_MIN, I64_MAX = -2**63, 2**63 - 1
I32_MIN, I32_MAX = -2**31, 2**31 - 1
NAN, INF = float("nan"), float("inf")

# columns: 0 bool, 1 int32, 2 int64, 3 float32, 4 float64 (+ a second of
# each numeric dtype at 5..8 so binary ops see unequal operands)
COLS = [
    torch.tensor([True, False, True, True, False, False, True, False]),
    torch.tensor([0, 1, -1, I32_MAX, I32_MIN, -7, 7, 123456],
                 dtype=torch.int32),
    torch.tensor([0, 1, -1, I64_MAX, I64_MIN, -7, 2**24 + 1, 3037000500],
                 dtype=torch.int64),
    torch.tensor([0.0, -0.0, 1.5, NAN, INF, -INF, -2.5, 1e-40],
                 dtype=torch.float32),
    torch.tensor([0.0, -0.0, 1.5, NAN, INF, -INF, -2.5, 1e-310],
                 dtype=torch.float64),
    torch.tensor([3, -3, I32_MAX, I32_MAX, -1, 2, -7, 0],
                 dtype=torch.int32),
    torch.tensor([3, -3, 2**62, I64_MAX, -1, 2, 3037000500, 0],
                 dtype=torch.int64),
    torch.tensor([NAN, 0.0, -1.5, 2.0, INF, 1.0, -2.5, 3.0],
                 dtype=torch.float32),
    torch.tensor([NAN, 0.0, -1.5, 2.0, INF, 1.0, -2.5, 3.0],
                 dtype=torch.float64),
]
SCHEMA = Schema([c.dtype for c in COLS])
B, I32, I64, F32, F64, J32, J64, G32, G64 = range(9)
PARTNER = {I32: J32, I64: J64, F32: G32, F64: G64}


def bits(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def same(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _matrix():
    """(name, expr builder over column getter c, same builder in torch)."""
    cases = []

    def add(name, fn):
        cases.append((name, fn))

    for i in (I32, I64, F32, F64):
        j = PARTNER[i]
        n = SCHEMA.dtypes[i]
        add(f"add-{n}", lambda c, i=i, j=j: c(i) + c(j))
        add(f"sub-{n}", lambda c, i=i, j=j: c(i) - c(j))
        add(f"mul-{n}", lambda c, i=i, j=j: c(i) * c(j))
        add(f"addlit-{n}", lambda c, i=i: c(i) + 3)
        add(f"rsub-{n}", lambda c, i=i: 3 - c(i))
        add(f"mullit-{n}", lambda c, i=i: 2.5 * c(i))
        add(f"neg-{n}", lambda c, i=i: -c(i))
        add(f"abs-{n}", lambda c, i=i: abs(c(i)))
        add(f"div-{n}", lambda c, i=i, j=j: c(i) / c(j))
        add(f"divlit-{n}", lambda c, i=i: c(i) / 3)
        add(f"rdiv-{n}", lambda c, i=i: 2 / c(i))
        for op in ("__eq__", "__ne__", "__lt__", "__le__", "__gt__",
                   "__ge__"):
            add(f"{op}-{n}",
                lambda c, i=i, j=j, op=op: getattr(c(i), op)(c(j)))
        add(f"ltlit-{n}", lambda c, i=i: c(i) < 0.5)
        add(f"rgelit-{n}", lambda c, i=i: 1 >= c(i))
    for i in (B, I32, I64):
        n = SCHEMA.dtypes[i]
        add(f"floordiv-{n}", lambda c, i=i: c(i) // 3)
        add(f"mod-{n}", lambda c, i=i: c(i) % 3)
        add(f"floordiv-pow2-{n}", lambda c, i=i: c(i) // 8)
        add(f"mod-pow2-{n}", lambda c, i=i: c(i) % 8)
        add(f"mod-one-{n}", lambda c, i=i: c(i) % 1)
        add(f"invert-{n}", lambda c, i=i: ~c(i))
    for i in (I32, I64):
        j = PARTNER[i]
        n = SCHEMA.dtypes[i]
        add(f"and-{n}", lambda c, i=i, j=j: c(i) & c(j))
        add(f"or-{n}", lambda c, i=i, j=j: c(i) | c(j))
        add(f"xor-{n}", lambda c, i=i, j=j: c(i) ^ c(j))
        add(f"andlit-{n}", lambda c, i=i: c(i) & 7)
        add(f"shl-{n}", lambda c, i=i: c(i) << 3)
        add(f"shr-{n}", lambda c, i=i: c(i) >> 3)
        add(f"shr-max-{n}",
            lambda c, i=i: c(i) >> (31 if i == I32 else 63))
    # bool logic, mixed widths, where, minimum/maximum, casts
    add("bool-and", lambda c: c(B) & (c(I32) > 0))
    add("bool-or-lit", lambda c: c(B) | False)
    add("bool-xor", lambda c: c(B) ^ (c(F32) > 0))
    add("bool-add", lambda c: c(B) + (c(I64) < 0))
    add("bool-mul", lambda c: c(B) * (c(I64) < 0))
    add("bool-plus-int", lambda c: c(B) + 1)
    add("bool-eq", lambda c: c(B) == (c(I32) > 0))
    add("i32-plus-i64", lambda c: c(I32) + c(I64))
    add("i32-and-i64", lambda c: c(I32) & c(I64))
    add("i64-times-f32", lambda c: c(I64) * c(F32))
    add("f32-plus-f64", lambda c: c(F32) + c(F64))
    add("i32-lt-f64", lambda c: c(I32) < c(F64))
    add("i32-wrap", lambda c: c(I32) * c(I32) + I32_MAX)
    add("i64-wrap", lambda c: c(I64) * c(J64) * 3 + 1)
    return cases


MATRIX = _matrix()
# (name, Expr builder, torch builder): the two differ only where the
# vocabulary spells a torch function differently
FUNCS = [
    ("where-mixed",
     lambda c: bs.where(c(F32) > 0, c(I32), 2.5),
     lambda c: torch.where(c(F32) > 0, c(I32), 2.5)),
    ("where-i32-f64",
     lambda c: bs.where(c(B), c(I32), c(F64)),
     lambda c: torch.where(c(B), c(I32), c(F64))),
    ("where-lits",
     lambda c: bs.where(c(B), 1, 0),
     lambda c: torch.where(c(B), 1, 0)),
    ("min-f32", lambda c: bs.minimum(c(F32), c(G32)),
     lambda c: torch.minimum(c(F32), c(G32))),
    ("max-f32", lambda c: bs.maximum(c(F32), c(G32)),
     lambda c: torch.maximum(c(F32), c(G32))),
    ("min-f64", lambda c: bs.minimum(c(F64), c(G64)),
     lambda c: torch.minimum(c(F64), c(G64))),
    ("max-f64", lambda c: bs.maximum(c(F64), c(G64)),
     lambda c: torch.maximum(c(F64), c(G64))),
    ("min-i64", lambda c: bs.minimum(c(I64), c(J64)),
     lambda c: torch.minimum(c(I64), c(J64))),
    ("max-i32-i64", lambda c: bs.maximum(c(I32), c(I64)),
     lambda c: torch.maximum(c(I32), c(I64))),
    ("min-lit", lambda c: bs.minimum(c(F32), 1.0),
     lambda c: torch.minimum(c(F32), torch.tensor(1.0))),
    ("max-lit-first", lambda c: bs.maximum(0, c(I32)),
     lambda c: torch.maximum(torch.tensor(0, dtype=torch.int32), c(I32))),
] + [
    (f"to-{SCHEMA.dtypes[i]}-{dt}",
     lambda c, i=i, dt=dt: c(i).to(dt),
     lambda c, i=i, dt=dt: c(i).to(dt))
    for i in (B, I32, I64, J32, J64)
    for dt in exprs.DTYPES
] + [
    # float -> int of NaN/inf/out-of-range is unspecified: finite rows
    (f"to-{SCHEMA.dtypes[i]}-{dt}",
     lambda c, i=i, dt=dt: bs.where(abs(c(i)) < 100, c(i), 7.25).to(dt),
     lambda c, i=i, dt=dt: torch.where(abs(c(i)) < 100, c(i), 7.25).to(dt))
    for i in (F32, F64)
    for dt in exprs.DTYPES
]
ALL = [(n, f, f) for n, f in MATRIX] + FUNCS


def _col(i):
    return bs.col(i, SCHEMA.dtypes[i])


@pytest.mark.parametrize("name,build,oracle", ALL, ids=[a[0] for a in ALL])
def test_eval_and_dtype_match_torch(name, build, oracle):
    e = build(_col)
    want = oracle(lambda i: COLS[i])
    assert e.dtype == want.dtype
    assert same(e.eval(COLS), want)
    # untyped columns type themselves from the schema
    assert build(bs.col).bind(SCHEMA).dtype == want.dtype


@pytest.mark.parametrize("name,build,oracle", ALL, ids=[a[0] for a in ALL])
def test_program_matches_eval(name, build, oracle):
    e = build(_col)
    p = compile_program([e], None, SCHEMA)
    assert p.eligible, p.reason
    outs, keep = run_program_host(p, COLS)
    assert keep is None
    assert same(outs[0], e.eval(COLS))


def test_named_edge_values():
    c = _col
    assert (c(I32) * c(I32) + I32_MAX).eval(COLS)[3].item() == \
        ((I32_MAX * I32_MAX + I32_MAX + 2**31) % 2**32) - 2**31
    assert (c(I64) * 3).eval(COLS)[3].item() == \
        ((I64_MAX * 3 + 2**63) % 2**64) - 2**63
    assert abs(c(I64)).eval(COLS)[4].item() == I64_MIN
    lt = c(I64) < 0.5
    assert lt.dtype == torch.bool
    # float32 promotion: 2**24 + 1 rounds to 2**24 before the compare
    assert (c(I64) == 16777216.0).eval(COLS)[6].item() is True
    assert (c(I64) // 3).eval(COLS)[5].item() == -3
    assert (c(I64) % 3).eval(COLS)[5].item() == 2
    assert (c(I32) >> 3).eval(COLS)[5].item() == -1
    assert (c(F32) == c(F32)).eval(COLS)[3].item() is False
    m = bs.minimum(c(F32), c(G32)).eval(COLS)
    assert torch.isnan(m[0]) and torch.isnan(m[3])


def _random_tree(rng, depth):
    if depth == 0 or rng.random() < 0.15:
        return _col(rng.choice([I32, I64, F32, F64, J32, J64, G32, G64]))
    a = _random_tree(rng, depth - 1)
    kind = rng.choice(["bin", "lit", "cmpw", "un", "int"])
    if kind == "bin":
        b = _random_tree(rng, depth - 1)
        return rng.choice([lambda: a + b, lambda: a - b, lambda: a * b,
                           lambda: bs.minimum(a, b),
                           lambda: bs.maximum(a, b)])()
    if kind == "lit":
        k = rng.choice([2, -3, 0.5, 7])
        return rng.choice([lambda: a + k, lambda: k - a, lambda: a * k])()
    if kind == "cmpw":
        b = _random_tree(rng, depth - 1)
        return bs.where(a < b, a, b)
    if kind == "un":
        return rng.choice([lambda: -a, lambda: abs(a)])()
    if a.dtype.is_floating_point:
        return a / 3
    return rng.choice([lambda: a // 5, lambda: a % 6, lambda: a >> 2,
                       lambda: a ^ 21, lambda: ~a])()


@pytest.mark.parametrize("seed", range(6))
def test_random_trees(seed):
    rng = random.Random(seed)
    outs = [_random_tree(rng, 5) for _ in range(2)]
    pred = _random_tree(rng, 3) > _random_tree(rng, 3)
    p = compile_program(outs, pred, SCHEMA)
    got, keep = run_program_host(p, COLS)   # runs eligible or not
    assert same(keep, pred.eval(COLS))
    for g, e in zip(got, outs):
        assert same(g, e.eval(COLS))


def test_shared_subexpression_is_lowered_once():
    x = _col(I64) * 3 + 1
    p = compile_program([x, x + x, (x + x) * x], (x & 7) != 0, SCHEMA)
    assert p.eligible
    out_section = p.instrs[p.n_pred:]
    muls = [i for i in out_section if i[0] == exprs.OP_MUL]
    adds = [i for i in out_section if i[0] == exprs.OP_ADD]
    assert len(muls) == 2 and len(adds) == 2     # x*3, (..)*x; +1, x+x
    got, keep = run_program_host(p, COLS)
    xs = COLS[I64] * 3 + 1
    assert same(keep, (xs & 7) != 0)
    assert same(got[2], (xs + xs) * xs)


def test_over_limit_program_is_not_eligible_but_still_runs():
    terms = [_col(I64) * (k + 2) for k in range(exprs.MAX_REGS + 2)]
    # a chain of xors consumes each term as it goes: registers are reused
    chain = terms[0]
    for t in terms[1:]:
        chain = chain ^ t
    assert compile_program([chain], None, SCHEMA).eligible
    # every term is needed again after the sum: they cannot share
    back = terms[0]
    for t in terms[1:]:
        back = back + t
    for t in terms:
        back = back ^ t
    p = compile_program([back], None, SCHEMA)
    assert not p.eligible and "MAX_REGS" in p.reason
    got, _ = run_program_host(p, COLS)
    assert same(got[0], back.eval(COLS))
    many = compile_program([_col(I64) + k for k in range(
        exprs.MAX_OUTPUTS + 1)], None, SCHEMA)
    assert not many.eligible and "MAX_OUTPUTS" in many.reason


def test_registers_follow_liveness():
    e = _col(I64)
    for k in range(20):
        e = (e + k) * 3
    p = compile_program([e], None, SCHEMA)
    assert p.eligible and p.nregs <= 2 and len(p.instrs) == 41


def test_passthrough_and_bytes():
    sch = Schema([torch.int64, BYTES, OBJECT])
    p = compile_program([bs.col(1), bs.col(0) + 1, bs.col(2), bs.col(0)],
                        None, sch)
    assert p.eligible
    assert [k for k, _ in p.outputs] == ["col", "reg", "col", "col"]
    assert p.inputs == [0]
    # a predicate has to move every output, so BYTES cannot ride along
    q = compile_program([bs.col(1), bs.col(0)], bs.col(0) > 0, sch)
    assert not q.eligible
    assert not compile_program(None, bs.col(0) > 0, sch).eligible
    assert compile_program(None, bs.col(0) > 0,
                           Schema([torch.int64, torch.float32])).eligible


def test_construction_errors():
    x, y = bs.col(0, torch.int64), bs.col(1, torch.int64)
    for bad in (lambda: x // y, lambda: x % y, lambda: x // 0,
                lambda: x % -3, lambda: x // 2.0, lambda: x // True,
                lambda: 7 // x, lambda: x << 64, lambda: x >> -1,
                lambda: bs.col(0, torch.int32) << 32, lambda: x << y,
                lambda: bs.col(0, torch.float32) << 1,
                lambda: bs.col(0, torch.float32) // 2,
                lambda: bs.col(0, BYTES) + 1,
                lambda: bs.col(0, OBJECT) == bs.col(1, OBJECT),
                lambda: bs.where(x, 1, 2), lambda: bs.col(-1),
                lambda: x.to(torch.int8), lambda: -bs.col(0, torch.bool),
                lambda: bs.minimum(1, 2), lambda: x + "a"):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(TypeError):
        bool(x > 0)
    # untyped columns: the same errors surface when the slice binds them
    src = bs.ReaderFunc(2, lambda shard, ctx: iter(()),
                        bs.schema_of(torch.int32, bytes))
    assert src.schema.dtypes == (torch.int32, BYTES)
    with pytest.raises(TypeError):
        bs.Map(src, bs.col(0) << 32)
    with pytest.raises(TypeError):
        bs.Map(src, bs.col(1) + 1)
    with pytest.raises(TypeError):
        bs.Map(src, bs.col(2))
    with pytest.raises(TypeError):
        bs.Filter(src, bs.col(2) > 0)
    with pytest.raises(TypeError):
        bs.Filter(src, bs.col(0) + 1)
    with pytest.raises(TypeError):
        bs.Map(src, bs.col(0) + 1, rowwise=True)
    with pytest.raises(TypeError):
        bs.Filter(src, bs.col(0) > 1, rowwise=True)
    with pytest.raises(TypeError):
        bs.Map(src, (bs.col(0), 3))
    with pytest.raises(TypeError):
        bs.Map(src, bs.col(0), out_schema=(int, int))


def test_map_schema():
    src = bs.Const(2, torch.arange(10, dtype=torch.int32),
                   torch.arange(10, dtype=torch.float64))
    m = bs.Map(src, (bs.col(1) * 2, bs.col(0) + 1, bs.col(0) < 3))
    assert m.schema == Schema([torch.float64, torch.int32, torch.bool], 1)
    assert bs.Map(src, bs.col(0) / 2).schema == Schema([torch.float32])
    m2 = bs.Map(src, (bs.col(0), bs.col(1)), out_schema=(int, float),
                prefix=2)
    assert m2.schema == Schema([torch.int64, torch.float64], 2)
    assert m2.exprs[0].dtype == torch.int64
    assert bs.Filter(src, bs.col(0) > 2).schema == src.schema


# -- engine level -----------------------------------------------------------

N = 5000


def _source(nshard, with_object=False):
    def gen(shard, ctx):
        g = torch.Generator()
        g.manual_seed(7 + shard)
        for _ in range(2):
            k = torch.randint(-1000, 1000, (N,), dtype=torch.int64,
                              generator=g)
            v = torch.randn(N, dtype=torch.float32, generator=g)
            if with_object:
                yield (k, v, [f"s{int(x)}" for x in k])
            else:
                yield (k, v)
    types = (int, torch.float32, str) if with_object \
        else (int, torch.float32)
    return bs.ReaderFunc(nshard, gen, bs.schema_of(*types))


CHAINS = {
    "map": (
        lambda s: bs.Map(s, (bs.col(0) * 3 + 1, bs.col(1) * 0.5)),
        lambda s: bs.Map(s, lambda k, v: (k * 3 + 1, v * 0.5))),
    "filter": (
        lambda s: bs.Filter(s, (bs.col(0) & 7) != 0),
        lambda s: bs.Filter(s, lambda k, v: (k & 7) != 0)),
    "map-filter": (
        lambda s: bs.Filter(bs.Map(s, (bs.col(0) * 3 + 1, bs.col(1))),
                            (bs.col(0) & 7) != 0),
        lambda s: bs.Filter(bs.Map(s, lambda k, v: (k * 3 + 1, v)),
                            lambda k, v: (k & 7) != 0)),
    "filter-map-filter": (
        lambda s: bs.Filter(
            bs.Map(bs.Filter(s, bs.col(1) > 0),
                   (bs.col(0) % 10, bs.col(1) + bs.col(0))),
            (bs.col(0) != 3) & (bs.col(1) < 500)),
        lambda s: bs.Filter(
            bs.Map(bs.Filter(s, lambda k, v: v > 0),
                   lambda k, v: (k % 10, v + k)),
            lambda k, v: (k != 3) & (v < 500))),
}


def _shard_rows(res):
    """Rows per shard, in stream order."""
    out = []
    for shard in range(res.num_shards):
        rows = []
        for f in res.reader(shard, [], None):
            rows.extend(zip(*f.column_lists()))
        out.append(rows)
    return out


def _run(build, nshard=3):
    sess = bs.start(parallelism=2, device="cpu")
    return sess.run(bs.func(build), nshard)


def _same_rows(a, b):
    ra, rb = _shard_rows(a), _shard_rows(b)
    assert len(ra) == len(rb)
    for x, y in zip(ra, rb):
        assert len(x) == len(y) and len(x) > 0
        assert str(x) == str(y)     # NaN-proof, order-sensitive
    assert sorted(map(str, a.scan())) == sorted(map(str, b.scan()))


@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_matches_lambdas(name):
    with_exprs, with_lambdas = CHAINS[name]
    _same_rows(_run(lambda n: with_exprs(_source(n))),
               _run(lambda n: with_lambdas(_source(n))))


def test_object_column_rides_through_a_filter():
    a = _run(lambda n: bs.Filter(_source(n, True), (bs.col(0) & 3) == 1))
    b = _run(lambda n: bs.Filter(_source(n, True),
                                 lambda k, v, s: (k & 3) == 1))
    _same_rows(a, b)
    row = next(iter(a.scan()))
    assert row[2] == f"s{row[0]}"
    # ... and through a Map as a bare column
    c = _run(lambda n: bs.Filter(
        bs.Map(_source(n, True), (bs.col(2), bs.col(0) + 1)),
        bs.col(1) > 0))
    row = next(iter(c.scan()))
    assert row[0] == f"s{row[1] - 1}"


class _Ctx:
    device = "cpu"


def _reader_chain(top):
    """Build the reader stack of a pipelined chain by hand, as the
    compiler's _make_do does, and return the top reader."""
    chain = []
    s = top
    while s.deps:
        chain.append(s)
        s = s.deps[0].slice
    reader = s.reader(0, [], _Ctx())
    for op in reversed(chain):
        reader = op.reader(0, [reader], _Ctx())
    return reader


def test_uninterrupted_chain_is_one_expr_reader():
    top = CHAINS["filter-map-filter"][0](_source(1))
    r = _reader_chain(top)
    assert isinstance(r, ExprReader)
    assert not isinstance(r.src, ExprReader)      # folded, not stacked
    assert r.spec.pred is not None and len(r.spec.outputs) == 2
    want = _reader_chain(CHAINS["filter-map-filter"][1](_source(1)))
    for got_f, want_f in zip(r, want):
        for g, w in zip(got_f.columns, want_f.columns):
            assert same(g, w)
        assert got_f.prefix == want_f.prefix
    # a lambda stage in between is a boundary: two readers
    mixed = bs.Filter(bs.Map(bs.Map(_source(1), (bs.col(0), bs.col(1))),
                             lambda k, v: (k, v)), bs.col(0) > 0)
    r = _reader_chain(mixed)
    assert isinstance(r, ExprReader) and not isinstance(r.src, ExprReader)
    assert r.spec.outputs is None


def test_started_reader_is_not_folded():
    inner = _reader_chain(bs.Map(_source(1), (bs.col(0) + 1, bs.col(1))))
    first = inner.read()
    assert first is not None and inner.started
    flt = bs.Filter(bs.Map(_source(1), (bs.col(0) + 1, bs.col(1))),
                    bs.col(0) > 0)
    outer = flt.reader(0, [inner], _Ctx())
    assert outer.src is inner


def test_materialize_is_a_boundary():
    seen = []
    orig = ExprReader.__init__

    def spy(self, src, spec):
        seen.append((spec.outputs is not None, spec.pred is not None))
        orig(self, src, spec)

    def build(n, cut):
        m = bs.Map(_source(n), (bs.col(0) * 3 + 1, bs.col(1)))
        if cut:
            m = bs.materialize(m)
        return bs.Filter(m, (bs.col(0) & 7) != 0)

    ExprReader.__init__ = spy
    try:
        cut = _run(lambda n: build(n, True), nshard=1)
        rows_cut = _shard_rows(cut)
        seen_cut, seen[:] = list(seen), []
        fused = _run(lambda n: build(n, False), nshard=1)
        rows_fused = _shard_rows(fused)
        seen_fused = list(seen)
    finally:
        ExprReader.__init__ = orig
    # with the boundary a map-only and a filter-only reader survive;
    # without it the last reader built holds both
    assert (True, False) in seen_cut and (False, True) in seen_cut
    assert (True, True) not in seen_cut
    assert seen_fused[-1] == (True, True)
    assert str(rows_cut) == str(rows_fused)


def test_filter_keeps_frame_metadata():
    from bigslice_amd.frame import Frame
    from bigslice_amd.sliceio import FrameReader
    f = Frame([torch.arange(10), torch.arange(10.0)], prefix=2,
              combined_id=41)
    src = bs.Const(1, torch.arange(10), torch.arange(10.0))
    flt = bs.Filter(src, bs.col(0) > 3)
    out = flt.reader(0, [FrameReader(f)], _Ctx()).read()
    want = f.mask(f.columns[0] > 3)
    assert (out.prefix, out.combined_id) == (want.prefix,
                                             want.combined_id) == (2, 41)
    m = bs.Map(src, (bs.col(1), bs.col(0)))
    out = m.reader(0, [FrameReader(f)], _Ctx()).read()
    assert (out.prefix, out.combined_id) == (1, None)
    assert out.columns[0].data_ptr() == f.columns[1].data_ptr()
    # an all-false filter yields no frame at all, like the lambda path
    none = bs.Filter(src, bs.col(0) < 0)
    assert none.reader(0, [FrameReader(f)], _Ctx()).read() is None
