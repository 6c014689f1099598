"""One key column through the shared key paths, on the device.

The tuple forms of kernels.sortedkeys and the one Cogroup device
generator serve one key column with the single-key kernels: the K18 run
pass, torch.searchsorted and the direct (key, value) radix sort.  Spies
on the extension see which bindings ran; results are compared with the
same functions on CPU tensors and with a CPU session."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

SPIED = ("runs_sorted", "runs_multi", "lex_searchsorted", "radix_sort_kv",
         "radix_argsort")


@pytest.fixture(scope="module")
def kernels():
    from bigslice_amd import kernels as k
    assert k.have_extension(), "HIP extension must be built in-tree"
    return k


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    monkeypatch.delenv("BIGSLICE_COGROUP_MULTIKEY", raising=False)


@pytest.fixture
def calls(kernels, monkeypatch):
    """{binding: [rows of its first argument, per call]}"""
    seen = {name: [] for name in SPIED}

    def spy_on(name):
        real = getattr(kernels._C, name)

        def spy(*a, **kw):
            first = a[0][0] if isinstance(a[0], (list, tuple)) else a[0]
            seen[name].append(first.shape[0])
            return real(*a, **kw)
        monkeypatch.setattr(kernels._C, name, spy)
    for name in SPIED:
        spy_on(name)
    return seen


def _sorted_keys(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-(n // 3) - 2, n // 3 + 2, (n,), dtype=torch.int64,
                      generator=g)
    return torch.sort(k).values.to(dtype)


def _through_tuple_forms(sk, k, other):
    """Every tuple form over the one column k (and, for the two-sided
    ones, the sorted-unique column `other`), as a flat list of tensors."""
    uniq, starts, ends = sk.runs_multi([k])
    out = [uniq[0], starts, ends, sk.unique_sorted_multi([k])[0]]
    for right in (False, True):
        out.append(sk.lex_searchsorted([uniq[0]], [other], right))
    out.append(sk.merge_sorted_unique_multi([uniq[0]], [other])[0])
    return out


# 4096 rows are one tile of runs_multi.hip, 4097 one row over
@pytest.mark.parametrize("n", [1, 4096, 4097])
def test_one_int64_column_runs_the_single_key_kernels(kernels, calls, n):
    from bigslice_amd.kernels import sortedkeys as sk
    k = _sorted_keys(n, torch.int64, n)
    other = torch.unique(_sorted_keys(n, torch.int64, n + 1))
    want = _through_tuple_forms(sk, k, other)
    assert not any(calls.values()), "the CPU path reached the extension"
    got = _through_tuple_forms(sk, k.to(DEV), other.to(DEV))
    assert calls["runs_sorted"], "the K18 run pass did not run"
    assert calls["runs_multi"] == [] and calls["lex_searchsorted"] == []
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w)


def test_one_int32_column_takes_the_mask_path(kernels, calls):
    from bigslice_amd.kernels import sortedkeys as sk
    k = _sorted_keys(4097, torch.int32, 7)
    other = torch.unique(_sorted_keys(4097, torch.int32, 8))
    want = _through_tuple_forms(sk, k, other)
    got = _through_tuple_forms(sk, k.to(DEV), other.to(DEV))
    assert not any(calls.values())
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w)


# -- Cogroup ------------------------------------------------------------------

def _side(n, nkey, nkeys, seed, nval=1):
    """nkey int64 key columns over about nkeys keys, nval int64 values."""
    g = torch.Generator().manual_seed(seed)
    hi = max(2, round(nkeys ** (1.0 / nkey)))
    cols = [torch.randint(0, hi, (n,), dtype=torch.int64, generator=g)
            for _ in range(nkey)]
    cols += [torch.randint(-10**6, 10**6, (n,), dtype=torch.int64,
                           generator=g) for _ in range(nval)]
    return cols


def _run(sides, nkey, device):
    import bigslice_amd as bs

    def job():
        return bs.Cogroup(*[bs.Prefixed(bs.Const(3, *cols), nkey)
                            for cols in sides])
    sess = bs.start(parallelism=2, device=device)
    rows = list(sess.run(bs.func(job)).scan())
    sess.shutdown()
    return sorted(tuple(r[:nkey]) + tuple(tuple(sorted(v))
                                          for v in r[nkey:])
                  for r in rows)


def _same_on_device(sides, nkey):
    want = _run(sides, nkey, "cpu")
    assert len(want) > 0
    assert _run(sides, nkey, DEV) == want
    return want


def test_single_key_cogroup_runs_the_single_key_kernels(calls):
    rows = _same_on_device([_side(3000, 1, 50, 1), _side(2000, 1, 50, 2)],
                           1)
    assert len(rows) == 50
    assert calls["radix_sort_kv"] and calls["runs_sorted"]
    assert calls["runs_multi"] == [] and calls["lex_searchsorted"] == []
    assert calls["radix_argsort"] == []


def test_single_key_cogroup_two_value_columns_sort_a_permutation(calls):
    # every row of the dep with two value columns goes through the
    # argsort, every row of the other through the (key, value) sort
    _same_on_device([_side(3000, 1, 50, 3, nval=2), _side(2000, 1, 50, 4)],
                    1)
    assert sum(calls["radix_argsort"]) == 3000
    assert sum(calls["radix_sort_kv"]) == 2000


def test_two_column_cogroup_never_runs_the_single_key_pass(calls):
    _same_on_device([_side(3000, 2, 50, 5), _side(2000, 2, 50, 6)], 2)
    assert calls["runs_multi"], "the multi-column device cogroup did not run"
    assert calls["runs_sorted"] == []


@pytest.mark.parametrize("nkey", [1, 2])
@pytest.mark.parametrize("empty", [0, 1, 2])
def test_three_deps_one_empty(nkey, empty):
    sides = [_side(1500, nkey, 40, 10 + i) for i in range(3)]
    sides[empty] = [c[:0] for c in sides[empty]]
    rows = _same_on_device(sides, nkey)
    # every value column of the empty dep (value columns follow the key
    # in dep order)
    nvals = [len(cols) - nkey for cols in sides]
    first = nkey + sum(nvals[:empty])
    assert all(len(v) == 0 for r in rows
               for v in r[first:first + nvals[empty]])
