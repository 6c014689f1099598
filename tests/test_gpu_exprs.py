"""The fused expression kernel (csrc/expr.hip) against Expr.eval on the
same device tensors, bit for bit, and Expr chains through the engine on a
GPU session against the lambda chains on a CPU session."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


def bits(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def same(a, b):
    return (a.dtype == b.dtype and a.shape == b.shape
            and torch.equal(bits(a), bits(b)))


def _schema(cols):
    from bigslice_amd.schema import Schema
    return Schema([c.dtype for c in cols])


def run_native(kernels, outputs, pred, cols):
    """One launch; returns (out_cols, count).  Asserts the native path is
    really taken."""
    from bigslice_amd.exprs import compile_program
    from bigslice_amd.frame import Frame
    p = compile_program(outputs, pred, _schema(cols))
    assert p.eligible, p.reason
    assert kernels.expr_supported(p, Frame(cols))
    return kernels.expr_apply(p, cols)


def check(kernels, outputs, pred, cols):
    import bigslice_amd as bs
    got, count = run_native(kernels, outputs, pred, cols)
    sch = _schema(cols)
    exprs = outputs if outputs is not None \
        else [bs.col(i) for i in range(len(cols))]
    want = [e.bind(sch).eval(cols) for e in exprs]
    if pred is None:
        assert count is None
    else:
        keep = pred.bind(sch).eval(cols)
        assert count == int(keep.sum())
        want = [w[keep] for w in want]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), f"output {i} differs at n={len(cols[0])}"
    return got


def sizes(kernels, extra=()):
    T = kernels.EXPR_TILE_ROWS
    return [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1,
            3 * T + 17] + list(extra)


# -- data -------------------------------------------------------------------

def ints(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    info = torch.iinfo(dtype)
    x = torch.randint(info.min // 2, info.max // 2, (n,), dtype=dtype,
                      generator=g) * 2 + 1
    small = torch.randint(-20, 20, (n,), dtype=dtype, generator=g)
    x = torch.where(torch.rand(n, generator=g) < 0.5, x, small)
    edge = torch.tensor([info.min, info.max, 0, -1, 1, -7, 7, info.min + 1],
                        dtype=dtype)
    k = min(n, len(edge))
    x[:k] = edge[:k]
    return x.to(DEV)


def floats(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, dtype=dtype, generator=g) * 50
    tiny = 1e-40 if dtype == torch.float32 else 1e-310
    edge = torch.tensor([float("nan"), -0.0, 0.0, float("inf"),
                         -float("inf"), tiny, -tiny, 1.5], dtype=dtype)
    k = min(n, len(edge))
    # edges at the END too, so row 0 is not the only NaN
    x[:k] = edge[:k]
    if n > 2 * k:
        x[-k:] = edge.flip(0)[:k]
    return x.to(DEV)


def bools(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) < 0.5).to(DEV)


def int_programs(c, other_dt):
    """Every opcode of an integer dtype; x = col 0, y = col 1."""
    import bigslice_amd as bs
    x, y = c(0), c(1)
    return [
        [x + y, x - y, x * y, -x],
        [abs(x), x // 7, x % 7, x // 16],
        [x & y, x | y, x ^ y, ~x],
        [x << 5, x >> 5, x % 32, 3 - x],
        [(x == y) | (x != y), (x < y) ^ (x <= y), (x > y) & (x >= y),
         bs.where(x > 0, x, 9)],
        [bs.minimum(x, y), bs.maximum(x, y), x * 3 + 1, (x & 7) != 0],
        [x.to(torch.bool), x.to(other_dt), x.to(torch.float32),
         x.to(torch.float64)],
        [x / y, x / 3, bs.minimum(x, 5), x < 0.5],
    ]


def float_programs(c, other_dt):
    import bigslice_amd as bs
    x, y = c(0), c(1)
    fin = bs.where(abs(x) < 100, x, 7.25)   # float->int needs finite
    return [
        [x + y, x - y, x * y, -x],
        [abs(x), x / y, x / 3, 2 / x],
        [x == y, x != y, x < y, x <= y],
        [x > y, x >= y, bs.where(x > y, x, 0.5), x * 0.1 + 1],
        [bs.minimum(x, y), bs.maximum(x, y), bs.minimum(x, 1.0),
         bs.maximum(y, x)],
        [x.to(torch.bool), x.to(other_dt), fin.to(torch.int32),
         fin.to(torch.int64)],
        [x == x, (x - x) * y, x + 1, (x * y + x) - y],
    ]


def bool_programs(c):
    import bigslice_amd as bs
    x, y = c(0), c(1)
    return [
        [x & y, x | y, x ^ y, ~x],
        [x == y, x < y, x + y, x * y],
        [x != y, x <= y, x > y, x >= y],
        [bs.where(x, y, True), x + 1, x.to(torch.int32),
         x.to(torch.float64)],
        [x.to(torch.int64), x.to(torch.float32), x | False, ~x ^ y],
    ]


@pytest.mark.parametrize("dtype", ["bool", "int32", "int64", "float32",
                                   "float64"])
def test_map_only_every_opcode(kernels, dtype):
    import bigslice_amd as bs
    dt = getattr(torch, dtype)
    for n in sizes(kernels):
        if dtype == "bool":
            cols = [bools(n, 1), bools(n, 2)]
            progs = bool_programs(bs.col)
        elif dtype.startswith("int"):
            cols = [ints(n, dt, 1), ints(n, dt, 2)]
            progs = int_programs(
                bs.col, torch.int64 if dt == torch.int32 else torch.int32)
        else:
            cols = [floats(n, dt, 1), floats(n, dt, 2).flip(0)]
            progs = float_programs(
                bs.col,
                torch.float64 if dt == torch.float32 else torch.float32)
        for outs in progs:
            check(kernels, outs, None, cols)


def test_every_opcode_is_exercised(kernels):
    """The program lists above really cover the opcode table, dtype by
    dtype (CONST/LOAD/CAST/WHERE count under the dtype they produce)."""
    import bigslice_amd as bs
    from bigslice_amd import exprs as ex
    from bigslice_amd.schema import Schema
    seen = set()
    for dt, progs, other in [
            (torch.int32, int_programs, torch.int64),
            (torch.int64, int_programs, torch.int32),
            (torch.float32, float_programs, torch.float64),
            (torch.float64, float_programs, torch.float32)]:
        for outs in progs(bs.col, other):
            p = ex.compile_program(outs, None, Schema([dt, dt]))
            seen |= {(i[0], ex.DTYPES[i[1]]) for i in p.instrs}
    for outs in bool_programs(bs.col):
        p = ex.compile_program(outs, None,
                               Schema([torch.bool, torch.bool]))
        seen |= {(i[0], ex.DTYPES[i[1]]) for i in p.instrs}
    common = [ex.OP_CONST, ex.OP_LOAD, ex.OP_CAST, ex.OP_WHERE] + \
        list(range(ex.OP_EQ, ex.OP_GE + 1))
    arith = [ex.OP_ADD, ex.OP_SUB, ex.OP_MUL, ex.OP_NEG, ex.OP_ABS,
             ex.OP_MIN, ex.OP_MAX]
    intops = [ex.OP_FLOORDIV, ex.OP_MOD, ex.OP_AND, ex.OP_OR, ex.OP_XOR,
              ex.OP_NOT, ex.OP_SHL, ex.OP_SHR]
    want = {(o, torch.bool) for o in common + [
        ex.OP_AND, ex.OP_OR, ex.OP_XOR, ex.OP_NOT]}
    for dt in (torch.int32, torch.int64):
        want |= {(o, dt) for o in common + arith + intops}
    for dt in (torch.float32, torch.float64):
        want |= {(o, dt) for o in common + arith + [ex.OP_DIV]}
    assert want - seen == set()


def test_offset_views_and_passthrough(kernels):
    import bigslice_amd as bs
    for n in sizes(kernels):
        a = ints(n + 5, torch.int32, 3)[3:3 + n]
        b = bools(n + 5, 4)[3:3 + n]
        c = ints(n + 1, torch.int64, 5)[1:]
        assert n == 0 or a.storage_offset() == 3 == b.storage_offset()
        cols = [a, b, c]
        outs = [bs.col(2), bs.where(bs.col(1), bs.col(0), -bs.col(0)),
                ~bs.col(1), bs.col(0) + bs.col(2)]
        got = check(kernels, outs, None, cols)
        assert got[0] is c                      # zero-copy pass-through
        check(kernels, outs, bs.col(1), cols)   # and compacted


PREDICATES = ["all", "none", "alternating", "random", "last", "first",
              "even-tiles"]


def _pred(name, n, T):
    import bigslice_amd as bs
    idx, rnd = bs.col(0), bs.col(2)
    return {
        "all": idx >= 0,
        "none": idx < 0,
        "alternating": (idx & 1) == 0,
        "random": rnd < 0.5,
        "last": idx == n - 1,
        "first": idx == 0,
        "even-tiles": ((idx // T) % 2) == 0,
    }[name]


@pytest.fixture(scope="module")
def filter_cols(kernels):
    """idx int64, int32 noise, float32 uniform: generated once at the
    largest size, sliced per case."""
    T = kernels.EXPR_TILE_ROWS
    n = 66 * T + 5
    g = torch.Generator().manual_seed(1234)
    return [torch.arange(n, dtype=torch.int64).to(DEV),
            torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32,
                          generator=g).to(DEV),
            torch.rand(n, dtype=torch.float32, generator=g).to(DEV)]


@pytest.mark.parametrize("name", PREDICATES)
def test_fused_map_filter(kernels, filter_cols, name):
    import bigslice_amd as bs
    T = kernels.EXPR_TILE_ROWS
    outs3 = [bs.col(0) * 3 + bs.col(1), bs.col(2) * 0.5]
    outs2 = [bs.col(1) ^ 21, bs.col(0) - bs.col(1)]
    for n in sizes(kernels, [66 * T + 5]):
        cols = [c[:n] for c in filter_cols]
        pred = _pred(name, n, T)
        got = check(kernels, outs3, pred, cols)
        if n:
            assert got[0].dtype == torch.int64 and \
                got[1].dtype == torch.float32
        if name != "random":    # two inputs: the int64 and the int32
            check(kernels, outs2, pred, cols[:2])


@pytest.mark.parametrize("name", PREDICATES)
def test_pure_filter(kernels, filter_cols, name):
    T = kernels.EXPR_TILE_ROWS
    for n in sizes(kernels, [66 * T + 5]):
        cols = [c[:n] for c in filter_cols]
        check(kernels, None, _pred(name, n, T), cols)


def test_state_is_rezeroed_between_launches(kernels, filter_cols):
    import bigslice_amd as bs
    T = kernels.EXPR_TILE_ROWS
    n = 5 * T + 3
    a = [c[:n] for c in filter_cols]
    b = [c[n:2 * n] for c in filter_cols]
    pred = (bs.col(1) & 3) != 0
    for cols in (a, b, a):
        check(kernels, None, pred, cols)


def test_selective_filter_returns_exact_size_tensors(kernels, filter_cols):
    import bigslice_amd as bs
    n = 200_000
    cols = [c[:n] for c in filter_cols]
    got = check(kernels, None, (bs.col(0) % 100) == 0, cols)
    assert len(got[0]) == n // 100
    for g in got:
        assert g.untyped_storage().nbytes() <= \
            2 * g.numel() * g.element_size()
    # an unselective one stays a view of the n-row allocation
    got = check(kernels, None, (bs.col(0) % 100) != 0, cols)
    assert got[0].untyped_storage().nbytes() == n * 8


# -- engine level -----------------------------------------------------------

def _spy(monkeypatch, kernels):
    calls = []
    orig = kernels.expr_apply

    def spy(program, cols):
        calls.append(len(cols[0]))
        return orig(program, cols)
    monkeypatch.setattr(kernels, "expr_apply", spy)
    return calls


def _chain_source(bs, nshard, rows=300_000):
    def gen(shard, ctx):
        g = torch.Generator()
        g.manual_seed(100 + shard)
        keys = torch.randint(0, 3000, (rows,), dtype=torch.int64,
                             generator=g)
        vals = torch.randint(1, 50, (rows,), dtype=torch.int64,
                             generator=g)
        yield (keys, vals)
    return bs.ReaderFunc(nshard, gen, bs.schema_of(int, int))


def test_chained_pipeline_exprs_gpu_matches_lambdas_cpu(kernels,
                                                        monkeypatch):
    import bigslice_amd as bs

    def with_lambdas(nshard):
        mapped = bs.Map(_chain_source(bs, nshard),
                        lambda k, v: (k, v * 2))
        filt = bs.Filter(mapped, lambda k, v: (k & 1) == 0)
        return bs.Map(bs.Reduce(filt, "sum"), lambda k, s: (k, s + 1))

    def with_exprs(nshard):
        mapped = bs.Map(_chain_source(bs, nshard),
                        (bs.col(0), bs.col(1) * 2))
        filt = bs.Filter(mapped, (bs.col(0) & 1) == 0)
        return bs.Map(bs.Reduce(filt, "sum"), (bs.col(0), bs.col(1) + 1))

    cpu = bs.start(parallelism=2, device="cpu").run(
        bs.func(with_lambdas), 4)
    calls = _spy(monkeypatch, kernels)
    gpu = bs.start(parallelism=2, device=DEV).run(bs.func(with_exprs), 4)
    assert sorted(cpu.scan()) == sorted(gpu.scan())
    # one launch per source batch for map+filter, not one per stage
    assert calls.count(300_000) == 4 and len(calls) >= 5


def test_bytes_column_takes_the_eval_path(kernels, monkeypatch):
    import bigslice_amd as bs
    from bigslice_amd.frame import BytesColumn

    def source(nshard, add):
        def gen(shard, ctx):
            g = torch.Generator()
            g.manual_seed(shard)
            k = torch.randint(0, 1000, (2000,), dtype=torch.int64,
                              generator=g)
            yield (k, k * 2 + add, BytesColumn.from_list(
                [b"w%d" % int(x) for x in k]))
        return bs.ReaderFunc(nshard, gen, bs.schema_of(int, int, bytes))

    def with_lambdas(nshard):
        return bs.Filter(source(nshard, 1), lambda k, v, w: (k & 1) == 0)

    def with_exprs(nshard):
        m = bs.Map(source(nshard, 0),
                   (bs.col(0), bs.col(1) + 1, bs.col(2)))
        return bs.Filter(m, (bs.col(0) & 1) == 0)

    cpu = bs.start(parallelism=2, device="cpu").run(
        bs.func(with_lambdas), 2)
    calls = _spy(monkeypatch, kernels)
    gpu = bs.start(parallelism=2, device=DEV).run(bs.func(with_exprs), 2)
    rows = sorted(gpu.scan())
    assert rows == sorted(cpu.scan()) and len(rows) > 100
    assert calls == []


def test_per_thread_streams(kernels, monkeypatch):
    import bigslice_amd as bs

    def with_lambdas(nshard):
        m = bs.Map(_chain_source(bs, nshard, 200_000),
                   lambda k, v: (k * 3 + 1, v))
        return bs.Filter(m, lambda k, v: (k & 7) != 0)

    def with_exprs(nshard):
        m = bs.Map(_chain_source(bs, nshard, 200_000),
                   (bs.col(0) * 3 + 1, bs.col(1)))
        return bs.Filter(m, (bs.col(0) & 7) != 0)

    cpu = bs.start(parallelism=4, device="cpu").run(
        bs.func(with_lambdas), 8)
    calls = _spy(monkeypatch, kernels)
    gpu = bs.start(parallelism=4, device=DEV).run(bs.func(with_exprs), 8)
    assert len(calls) == 8
    want, got = list(cpu.scan()), list(gpu.scan())
    assert len(got) == len(want) > 0
    assert sorted(got) == sorted(want)


@pytest.mark.parametrize("width", ["narrow", "medium", "wide"])
def test_register_file_widths(kernels, filter_cols, width):
    """The kernel interprets 4, 2 or 1 rows per decode depending on how
    many registers the program names (<= 4, <= 8, <= 16): cover each."""
    import bigslice_amd as bs
    from bigslice_amd.exprs import compile_program
    T = kernels.EXPR_TILE_ROWS
    x, y, z = bs.col(0), bs.col(1), bs.col(2)
    if width == "narrow":
        outs, lo, hi = [x * 3 + y], 1, 4
    elif width == "medium":
        outs, lo, hi = [x + y, x - y, x * y, z * 2.0], 5, 8
    else:
        t = [x * (k + 2) + y for k in range(9)]
        acc = t[0]
        for v in t[1:]:
            acc = acc + v
        for v in t:
            acc = acc ^ v
        outs, lo, hi = [acc, z + 1, x - y, y >> 1], 9, 16
    pred = ((x & 3) != 1) & (z < 0.9)
    for n in (T + 1, 3 * T + 17):
        cols = [c[:n] for c in filter_cols]
        for p in (None, pred):
            prog = compile_program(outs, p, _schema(cols))
            assert lo <= prog.nregs <= hi, prog.nregs
            check(kernels, outs, p, cols)
