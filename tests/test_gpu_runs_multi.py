"""Run boundaries, lexicographic search and lexicographic sort over
multi-column keys on the device (K22, csrc/runs_multi.hip).

Every comparison is torch.equal against a CPU oracle that never calls
the code under test: a diff mask over the stacked columns for the runs,
bisect over Python tuples for the search, the torch.sort chain for the
sort."""

import bisect

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1


@pytest.fixture(scope="module")
def sk():
    from bigslice_amd import kernels
    assert kernels.have_extension(), "HIP extension must be built in-tree"
    from bigslice_amd.kernels import sortedkeys
    return sortedkeys


def _oracle_runs(cols):
    """(uniq columns, starts, ends) of sorted CPU columns."""
    n = cols[0].shape[0]
    flag = torch.zeros(n, dtype=torch.bool)
    if n:
        flag[0] = True
    for c in cols:
        flag[1:] |= c[1:] != c[:-1]
    starts = flag.nonzero().flatten()
    ends = torch.cat([starts[1:], torch.tensor([n], dtype=torch.int64)])
    return [c[starts] for c in cols], starts, ends


def _check_runs(sk, cols):
    n = cols[0].shape[0]
    want_u, want_s, want_e = _oracle_runs(cols)
    uniq, starts, ends = sk.runs_multi([c.to(DEV) for c in cols])
    assert len(uniq) == len(cols)
    for g, w in zip(uniq, want_u):
        assert g.dtype == w.dtype
        assert torch.equal(g.cpu(), w)
    assert torch.equal(starts.cpu(), want_s)
    assert torch.equal(ends.cpu(), want_e)
    # starts and ends partition [0, n)
    s, e = starts.cpu(), ends.cpu()
    assert int(s[0]) == 0 and int(e[-1]) == n
    assert torch.equal(s[1:], e[:-1]) and bool((e > s).all())
    got_u = sk.unique_sorted_multi([c.to(DEV) for c in cols])
    for g, w in zip(got_u, want_u):
        assert torch.equal(g.cpu(), w)


def _from_run_ids(ids, ncols, vary):
    """Sorted columns whose tuple changes exactly where ids changes; only
    column `vary` carries the change, the others are constant."""
    return [ids.clone() if c == vary else torch.full_like(ids, 5)
            for c in range(ncols)]


def _sizes(sk):
    T = sk.MRUNS_TILE_ROWS
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


@pytest.mark.parametrize("ncols", [2, 3, 4, 5, 8])
def test_runs_random_over_sizes(sk, ncols):
    g = torch.Generator().manual_seed(ncols)
    for n in _sizes(sk):
        # ~n/3 distinct tuples: runs of a few rows, many crossing lanes
        ids = torch.sort(torch.randint(0, n // 3 + 1, (n,),
                                       dtype=torch.int64,
                                       generator=g)).values
        # spread the id over the columns, most significant first
        cols = [(ids // (3 ** (ncols - 1 - c))) % 3 if c else
                ids // (3 ** (ncols - 1)) for c in range(ncols)]
        _check_runs(sk, cols)


@pytest.mark.parametrize("ncols", [2, 3, 4, 5, 8])
def test_runs_boundary_at_wave_and_tile_edges(sk, ncols):
    T = sk.MRUNS_TILE_ROWS
    n = 3 * T + 17
    r = torch.arange(n)
    for vary in (0, ncols - 1):
        # a boundary exactly at row 64 and exactly at row T, nowhere else
        ids = (r >= 64).to(torch.int64) + (r >= T).to(torch.int64)
        _check_runs(sk, _from_run_ids(ids, ncols, vary))
        # no boundary at either: the runs cross the wave and tile edges
        ids = (r >= 70).to(torch.int64) + (r >= T + 9).to(torch.int64)
        _check_runs(sk, _from_run_ids(ids, ncols, vary))
        # a boundary at the first row of every wave
        _check_runs(sk, _from_run_ids(r // 64, ncols, vary))


@pytest.mark.parametrize("ncols", [2, 3, 4, 5, 8])
def test_runs_single_column_differences(sk, ncols):
    n = 2 * sk.MRUNS_TILE_ROWS + 65
    r = torch.arange(n)
    # rows differ only in the last column
    _check_runs(sk, _from_run_ids(r // 3, ncols, ncols - 1))
    # rows differ only in the first column while the last repeats,
    # (1,5),(2,5): catches a flag taken from one column
    _check_runs(sk, _from_run_ids(r // 2, ncols, 0))
    # all rows equal: one run
    cols = [torch.full((n,), 7, dtype=torch.int64) for _ in range(ncols)]
    _check_runs(sk, cols)
    uniq, starts, ends = sk.runs_multi([c.to(DEV) for c in cols])
    assert starts.cpu().tolist() == [0] and ends.cpu().tolist() == [n]
    # all rows distinct: n runs
    _check_runs(sk, _from_run_ids(r, ncols, ncols - 1))
    uniq, starts, ends = sk.runs_multi(
        [c.to(DEV) for c in _from_run_ids(r, ncols, 0)])
    assert torch.equal(starts.cpu(), r)


@pytest.mark.parametrize("ncols", [2, 3, 4, 5, 8])
def test_runs_int64_extremes_adjacent(sk, ncols):
    for col in range(ncols):
        base = [torch.zeros(130, dtype=torch.int64) for _ in range(ncols)]
        base[col][:65] = INT64_MIN
        base[col][65:] = INT64_MAX
        _check_runs(sk, base)
        uniq, starts, _ = sk.runs_multi([c.to(DEV) for c in base])
        assert starts.cpu().tolist() == [0, 65]
        assert uniq[col].cpu().tolist() == [INT64_MIN, INT64_MAX]


def test_runs_empty_and_int32(sk):
    e = [torch.empty(0, dtype=torch.int64, device=DEV) for _ in range(2)]
    uniq, starts, ends = sk.runs_multi(e)
    assert [u.shape[0] for u in uniq] == [0, 0]
    assert starts.shape[0] == ends.shape[0] == 0
    a = torch.tensor([1, 1, 2, 2, 2], dtype=torch.int32)
    b = torch.tensor([5, 6, 6, 6, 7], dtype=torch.int64)
    _check_runs(sk, [a, b])


def test_runs_one_readback(sk, monkeypatch):
    """runs_multi reads one scalar back per call, as runs() does."""
    n = sk.MRUNS_TILE_ROWS + 5
    cols = [torch.arange(n, device=DEV) // 4, torch.zeros(n, dtype=torch.int64,
                                                          device=DEV)]
    reads = []
    real = torch.Tensor.item

    def spy(self):
        reads.append(1)
        return real(self)
    monkeypatch.setattr(torch.Tensor, "item", spy)
    sk.runs_multi(cols)
    assert len(reads) == 1


# -- search -----------------------------------------------------------------

def _check_search(sk, srt, qs, ncols):
    def cols(rows):
        if not rows:
            return [torch.empty(0, dtype=torch.int64) for _ in range(ncols)]
        return [torch.tensor([r[c] for r in rows], dtype=torch.int64)
                for c in range(ncols)]
    s_dev = [c.to(DEV) for c in cols(srt)]
    q_dev = [c.to(DEV) for c in cols(qs)]
    for right, fn in ((False, bisect.bisect_left),
                      (True, bisect.bisect_right)):
        got = sk.lex_searchsorted(s_dev, q_dev, right=right)
        want = torch.tensor([fn(srt, q) for q in qs], dtype=torch.int64)
        assert got.dtype == torch.int64 and got.is_cuda
        assert torch.equal(got.cpu(), want), (ncols, right)


def _random_rows(n, ncols, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return [tuple(r) for r in torch.randint(
        lo, hi, (n, ncols), dtype=torch.int64, generator=g).tolist()]


@pytest.mark.parametrize("ncols", [2, 3, 4, 5, 8])
def test_search_matches_bisect(sk, ncols):
    # negative first-column values (signed compare); few values per
    # column, so ties in the leading columns are decided by the last
    srt = sorted(_random_rows(700, ncols, -3, 3, ncols))
    qs = (_random_rows(300, ncols, -4, 4, 50 + ncols)   # present + absent
          + srt[::5] + srt[::5]                          # duplicated
          + [(-9,) * ncols, (INT64_MIN,) * ncols]        # below every tuple
          + [(9,) * ncols, (INT64_MAX,) * ncols])        # above every tuple
    _check_search(sk, srt, qs, ncols)


def test_search_ties_decided_by_the_last_column(sk):
    srt = [(-3, 9), (4, 1), (4, 3), (4, 3), (4, 5)]
    qs = [(4, 0), (4, 3), (4, 3), (4, 4), (4, 6), (-3, 10), (-4, 0),
          (INT64_MIN, INT64_MAX), (INT64_MAX, INT64_MIN)]
    _check_search(sk, srt, qs, 2)


@pytest.mark.parametrize("u", [0, 1, 127, 128, 129, 1023, 1025])
def test_search_sizes(sk, u):
    srt = sorted(_random_rows(u, 2, -40, 40, u))
    qs = _random_rows(200, 2, -41, 41, u + 1) + srt[:50]
    _check_search(sk, srt, qs, 2)
    _check_search(sk, srt, [], 2)  # m == 0


# -- sort ---------------------------------------------------------------------

def _cpu_chain(cols):
    perm = torch.arange(cols[0].shape[0])
    for c in reversed(cols):
        perm = perm[torch.sort(c[perm], stable=True).indices]
    return perm


@pytest.mark.parametrize("ncols", [2, 3, 5])
def test_lex_argsort_equals_cpu_chain(sk, ncols):
    g = torch.Generator().manual_seed(30 + ncols)
    n = 20_011
    cols = [torch.randint(-50, 50, (n,), dtype=torch.int64, generator=g)
            for _ in range(ncols)]
    got = sk.lex_argsort([c.to(DEV) for c in cols])
    assert got.dtype == torch.int64
    assert torch.equal(got.cpu(), _cpu_chain(cols))


def test_lex_argsort_takes_an_int32_column(sk):
    g = torch.Generator().manual_seed(40)
    n = 9_001
    cols = [torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int64,
                          generator=g).to(torch.int32),
            torch.randint(-2**62, 2**62, (n,), dtype=torch.int64,
                          generator=g)]
    cols[0][::3] = 7  # ties in the int32 column, decided by the int64 one
    got = sk.lex_argsort([c.to(DEV) for c in cols])
    assert torch.equal(got.cpu(), _cpu_chain(cols))


@pytest.mark.parametrize("spread", [1, 65537])
def test_lex_argsort_is_stable(sk, spread):
    """Many duplicates in the leading column, and many fully equal
    tuples: equal tuples keep their input order, which only holds if
    every per-column radix argsort is stable.  The radix sort has two
    engines, chosen by which key bytes vary: spread 1 varies byte 0
    alone (a contiguous byte range, the rocPRIM engine), spread 65537
    varies bytes 0 and 2 around a constant byte 1 (the hand-written
    scatter)."""
    g = torch.Generator().manual_seed(41)
    n = 50_003
    cols = [torch.randint(0, 4, (n,), dtype=torch.int64, generator=g),
            torch.randint(0, 3, (n,), dtype=torch.int64, generator=g)]
    got = sk.lex_argsort([c.to(DEV) * spread for c in cols]).cpu()
    assert torch.equal(got, _cpu_chain(cols))
    # spelled out: inside one tuple value the row ids ascend
    tup = cols[0][got] * 3 + cols[1][got]
    same = tup[1:] == tup[:-1]
    assert bool((got[1:][same] > got[:-1][same]).all())
