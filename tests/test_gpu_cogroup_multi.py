"""Device Cogroup over multi-column integer keys (K22), end to end.

Every case runs the same bs.Cogroup on a CPU session (the host dict
path, the oracle) and on cuda:0, and compares the rows normalised as in
test_cogroup_device_matches_cpu: value lists sorted, rows sorted."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    monkeypatch.delenv("BIGSLICE_COGROUP_MULTIKEY", raising=False)


def _side(n, nkey, hi, seed, key_dtypes=None, val_dtypes=(torch.int64,)):
    """nkey key columns with values in [-hi, hi) and the value columns."""
    g = torch.Generator().manual_seed(seed)
    key_dtypes = key_dtypes or [torch.int64] * nkey
    keys = [torch.randint(-hi, hi, (n,), dtype=torch.int64,
                          generator=g).to(dt) for dt in key_dtypes]
    vals = []
    for dt in val_dtypes:
        v = torch.randint(-10**6, 10**6, (n,), dtype=torch.int64,
                          generator=g)
        vals.append(v.to(dt))
    return keys + vals


def _run(sides, nkey, device, raw=False):
    import bigslice_amd as bs

    def job():
        return bs.Cogroup(*[bs.Prefixed(bs.Const(3, *cols), nkey)
                            for cols in sides])
    sess = bs.start(parallelism=2, device=device)
    rows = list(sess.run(bs.func(job)).scan())
    sess.shutdown()
    if raw:
        return rows
    return _norm(rows, nkey)


def _norm(rows, nkey):
    return sorted(tuple(r[:nkey]) + tuple(tuple(sorted(v))
                                          for v in r[nkey:])
                  for r in rows)


def _same_on_device(sides, nkey):
    want = _run(sides, nkey, "cpu")
    got = _run(sides, nkey, DEV)
    assert len(want) > 0
    assert got == want
    return want


def test_two_column_keys_two_deps():
    # 4000 + 3000 rows over at most 20 x 20 tuples
    rows = _same_on_device([_side(4000, 2, 10, 1), _side(3000, 2, 10, 2)], 2)
    assert 300 <= len(rows) <= 400


def test_three_column_keys():
    _same_on_device([_side(3000, 3, 4, 3), _side(2500, 3, 4, 4)], 3)


def test_three_deps():
    _same_on_device([_side(2000, 2, 9, 5), _side(1500, 2, 9, 6),
                     _side(1000, 2, 9, 7)], 2)


def test_int32_key_column_keeps_output_dtypes():
    import bigslice_amd as bs
    dts = [torch.int32, torch.int64]
    sides = [_side(2000, 2, 8, 8, key_dtypes=dts),
             _side(1500, 2, 8, 9, key_dtypes=dts)]
    _same_on_device(sides, 2)

    # the frames the reader emits carry the input key dtypes
    def job():
        return bs.Cogroup(*[bs.Prefixed(bs.Const(1, *cols), 2)
                            for cols in sides])
    sess = bs.start(parallelism=1, device=DEV)
    frames = [f for f in sess.run(bs.func(job)).open() if len(f)]
    sess.shutdown()
    assert frames
    for f in frames:
        assert [c.dtype for c in f.columns[:2]] == dts


def test_tuples_present_in_only_one_dep():
    a = _side(1500, 2, 6, 10)
    b = _side(1500, 2, 6, 11)
    # disjoint in the second key column, shared in the first
    a[1] = a[1].abs() + 1
    b[1] = -(b[1].abs()) - 1
    rows = _same_on_device([a, b], 2)
    assert all((len(r[2]) == 0) != (len(r[3]) == 0) for r in rows)
    # and a partial overlap
    b[1][::2] = a[1][:1500:2]
    rows = _same_on_device([a, b], 2)
    assert any(len(r[2]) and len(r[3]) for r in rows)
    assert any(len(r[2]) == 0 or len(r[3]) == 0 for r in rows)


def test_one_dep_empty():
    a = _side(2000, 2, 7, 12)
    b = [c[:0] for c in _side(4, 2, 7, 13)]
    rows = _same_on_device([a, b], 2)
    assert all(len(r[3]) == 0 for r in rows)
    rows = _same_on_device([b, a], 2)
    assert all(len(r[2]) == 0 for r in rows)


def test_two_value_columns_of_different_dtypes():
    a = _side(2000, 2, 7, 14, val_dtypes=(torch.int64, torch.float32))
    b = _side(1500, 2, 7, 15, val_dtypes=(torch.int32,))
    _same_on_device([a, b], 2)


def test_switch_off_gives_equal_results(kernels, monkeypatch):
    """The device path runs (a spy on _C.runs_multi sees it), the host
    path under BIGSLICE_COGROUP_MULTIKEY=0 does not, and both agree with
    the CPU session."""
    calls = []
    real = kernels._C.runs_multi

    def spy(*a, **kw):
        calls.append(a[0][0].shape[0])
        return real(*a, **kw)
    monkeypatch.setattr(kernels._C, "runs_multi", spy)
    sides = [_side(3000, 2, 10, 16), _side(2000, 2, 10, 17)]
    want = _run(sides, 2, "cpu")
    assert calls == []
    got = _run(sides, 2, DEV)
    assert calls, "the multi-column device cogroup did not run"
    assert got == want
    ran = len(calls)
    monkeypatch.setenv("BIGSLICE_COGROUP_MULTIKEY", "0")
    assert _run(sides, 2, DEV) == want
    assert len(calls) == ran


def test_keys_come_back_in_lexicographic_order():
    sides = [_side(2000, 2, 9, 18), _side(1000, 2, 9, 19)]
    import bigslice_amd as bs

    def job():
        return bs.Cogroup(*[bs.Prefixed(bs.Const(1, *cols), 2)
                            for cols in sides])
    sess = bs.start(parallelism=1, device=DEV)
    keys = [tuple(r[:2]) for r in sess.run(bs.func(job)).scan()]
    sess.shutdown()
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
