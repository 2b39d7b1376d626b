"""The NumPy restatement of the favourites (tests/favourites_restatement.py) against ``oracle/recs_oracle.favourites``,
the properties the tables of tests/test_favourites_gpu.py promise, and the size of the favourites workspace.  No GPU."""
import numpy as np
import pytest

import favourites_restatement as F
from oracle import recs_oracle as orc


def _same_as_oracle(u, a, r, n_users, n_anime, pct):
    thr_o, fav_o = orc.favourites(u, a, r, n_users, pct)
    thr, bits = F.favourites(u, a, r, n_users, n_anime, pct)
    assert np.array_equal(np.isnan(thr), np.isnan(thr_o))
    assert np.array_equal(F.canon(thr), F.canon(thr_o)), pct           # bit for bit after + 0.0
    assert bits.dtype == np.uint32 and bits.shape == (n_users, (n_anime + 31) // 32)
    assert np.array_equal(bits, F.pack_sets(fav_o, n_anime)), pct      # the favourite sets


# ---------------------------------------------------------------- restatement == oracle
SIZES = (1, 2, 0, 63, 64, 65, 0, 0, 1023, 1024, 1025, 3000, 7, 70000, 0)


def _ratings(kind, rng, n):
    if kind == "grid":
        return rng.integers(0, 11, n) / 10
    if kind == "random":
        return rng.random(n)
    if kind == "negative":                                   # test_recs_gpu.py: sign and exponent bytes vary, -0.0 / 0.0
        r = rng.normal(0, 1e3, n) * (rng.random(n) > .2)
        r[::17] = -0.0
        return r
    return np.where(rng.random(n) < .5, 0.7, 0.7000000000000001)       # two_values


@pytest.mark.parametrize("kind", ["grid", "random", "negative", "two_values"])
def test_restatement_equals_the_oracle_at_segment_lengths(kind):
    rng = np.random.default_rng(41)
    n_users, n_anime = len(SIZES), 3000
    u = np.repeat(np.arange(n_users), SIZES).astype(np.int32)
    a = rng.integers(0, n_anime, len(u)).astype(np.int32)
    r = _ratings(kind, rng, len(u)).astype(np.float64)
    p = rng.permutation(len(u))
    for pct in F.PERCENTILES:
        _same_as_oracle(u, a, r, n_users, n_anime, pct)
    _same_as_oracle(u[p], a[p], r[p], n_users, n_anime, 37.5)          # the row order is nothing to either


@pytest.mark.parametrize("grid", [True, False])
def test_restatement_equals_the_oracle_on_many_short_users(grid):
    rng = np.random.default_rng(3)
    n_users, n_anime = 1500, 1500
    sizes = rng.integers(0, 90, n_users)
    sizes[:6] = [0, 1, 2, 3, 5, 300]
    u = np.repeat(np.arange(n_users), sizes).astype(np.int32)
    a = rng.integers(0, n_anime, len(u)).astype(np.int32)
    r = _ratings("grid" if grid else "random", rng, len(u))
    for pct in F.PERCENTILES:
        _same_as_oracle(u, a, r, n_users, n_anime, pct)


def test_restatement_of_an_empty_table():
    none = np.zeros(0, np.int32)
    thr_o, fav_o = orc.favourites(none, none, np.zeros(0), 5)
    thr, bits = F.favourites(none, none, np.zeros(0), 5, 40)
    assert np.isnan(thr_o).all() and fav_o == [set()] * 5
    assert np.isnan(thr).all() and thr.shape == (5,) and bits.shape == (5, 2) and not bits.any()


def test_dense_users_keeps_the_order_of_the_ids():
    u = np.array([4_000_000, 7, 7, 123_456, 4_000_000, 9], np.int32)
    ids, dense = F.dense_users(u)
    assert ids.tolist() == [7, 9, 123_456, 4_000_000] and dense.tolist() == [3, 0, 0, 2, 3, 1]
    assert np.array_equal(ids[dense], u)


def test_subset_oracle_is_the_oracle_of_those_users():
    table = F.scan_small_table(F.TILE - 1)
    users = np.array([0, 5, 17, 4000, F.TILE - 2])
    ids, thr, bits = F.subset_oracle(table, users, F.SCAN_ANIME)
    thr_all, bits_all = F.favourites(*table, F.TILE - 1, F.SCAN_ANIME)
    assert np.array_equal(ids, users)
    assert np.array_equal(F.canon(thr), F.canon(thr_all[users])) and np.array_equal(bits, bits_all[users])


# ---------------------------------------------------------------- the tables of the GPU file
def _descents(u):
    return (np.nonzero(np.diff(u.astype(np.int64)) < 0)[0] + 1).tolist()


def _neighbours_differ(thr):
    """Consecutive non-empty users have different thresholds: a segment read one row off, which takes a rating of the
    neighbour for one of its own, then shows in the threshold (a condition on the inputs, met exactly)."""
    t = thr[~np.isnan(thr)]
    assert len(t) > 1 and (t[1:] != t[:-1]).all()


@pytest.mark.parametrize("n_users", F.SCAN_SMALL_USERS)
def test_small_scan_tables(n_users):
    u, a, r = F.scan_small_table(n_users)
    cnt = np.bincount(u, minlength=n_users)
    assert len(cnt) == n_users and cnt.min() == 1 and cnt.max() == 12 and _descents(u) == []
    assert a.min() >= 0 and a.max() < F.SCAN_ANIME
    thr_o, _ = orc.favourites(u, a, r, n_users)
    _neighbours_differ(thr_o)
    assert _descents(F.shuffled((u, a, r), 1)[0])


@pytest.mark.parametrize("n_users", F.SCAN_LARGE_USERS)
def test_large_scan_tables(n_users):
    users = F.scan_large_users(n_users)
    n_tiles = (n_users + F.TILE - 1) // F.TILE
    assert n_tiles == {F.SCAN_LARGE_USERS[0]: 65, F.SCAN_LARGE_USERS[1]: 1025}[n_users]
    for t in (0, 1, 2, 62, 63, 64, 1022, 1023, 1024):
        if t < n_tiles:
            assert t * F.TILE in users and min(t * F.TILE + F.TILE - 1, n_users - 1) in users
    assert users[-1] == n_users - 1 and 2900 < len(users) < 3030
    u, a, r = table = F.scan_large_table(n_users)
    assert np.array_equal(np.unique(u), users) and _descents(u) == [] and u.max() == n_users - 1
    ids, thr, _ = F.subset_oracle(table, users, F.SCAN_ANIME)
    assert np.array_equal(ids, users)
    _neighbours_differ(thr)
    thr_r, _ = F.favourites(u, a, r, n_users, F.SCAN_ANIME)             # the restatement takes the huge range itself
    assert np.array_equal(F.canon(thr_r[users]), F.canon(thr)) and np.isnan(thr_r).sum() == n_users - len(users)


@pytest.mark.parametrize("tail", F.BREAK_TAILS)
def test_break_tables_have_one_descent_at_the_stated_row(tail):
    n = 3 * 4096 + tail
    u, a, r = F.break_table(tail, F.SCAN_ANIME)
    assert len(u) == n and _descents(u) == [] and u[0] == 1 and u[-1] == F.BREAK_USERS - 1
    cnt = np.bincount(u, minlength=F.BREAK_USERS)
    assert cnt[0] == 0 and cnt[1:].min() >= 120 and cnt[1:].max() <= 290
    begins = np.nonzero(np.diff(u))[0] + 1
    assert len(begins) == F.BREAK_USERS - 2 and not np.isin(begins % 256, (1, 2, 3)).any()
    thr_o, _ = orc.favourites(u, a, r, F.BREAK_USERS)
    _neighbours_differ(thr_o)
    want = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, n - 2, n - 1)
    assert F.break_positions(tail) == want and F.break_unfused_positions(tail) == (256, 1024, 4096, n - 1)
    for n_anime, positions in ((F.SCAN_ANIME, want), (F.BREAK_UNFUSED_ANIME, F.break_unfused_positions(tail))):
        for p in positions:
            ub, ab, rb = F.break_table(tail, n_anime, p)
            assert _descents(ub) == [p] and ub[p] == 0 and (ub != 0).sum() == n - 1
            assert ab.min() >= 0 and ab.max() == n_anime - 1
            if n_anime == F.SCAN_ANIME:
                assert np.array_equal(ab, a) and np.array_equal(rb, r)
    assert F.break_high_positions(tail) == want[:-2]
    for p in want[:-2]:
        ub, ab, rb = F.break_table(tail, F.SCAN_ANIME, p, high=True)
        assert _descents(ub) == [p] and ub[p - 1] == F.BREAK_USERS - 1 and ub[p] == u[p] and (ub != u).sum() == 1
        assert np.array_equal(ab, a) and np.array_equal(rb, r)
    assert (F.BREAK_UNFUSED_ANIME + 31) // 32 == F.FUSE_WORDS + 1


@pytest.mark.parametrize("lead", F.RUN_LEADS)
def test_run_tables_have_the_stated_run_starts(lead):
    lengths = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1, 1, 1, 1023, 1024, 1025, 2, 4093, 4096, 4099, 3, 20000, 1,
               70000, 1, 1)
    assert F.RUN_LENGTHS == lengths
    for grid in (True, False):
        (u, a, r), n_users = F.run_table(lead, grid)
        assert _descents(u) == [] and len(u) == lead + sum(lengths) and u.max() < n_users
        first = np.nonzero(np.r_[True, u[1:] != u[:-1]])[0]             # where a run of equal users begins
        runs = np.diff(np.r_[first, len(u)])
        assert runs.tolist() == [1] * lead + list(lengths)
        starts = first[lead:]
        assert np.array_equal(starts, F.run_starts(lead))
        assert np.array_equal(starts % 4, (lead + np.cumsum((0,) + lengths[:-1])) % 4)
        assert len(np.setdiff1d(np.arange(n_users), u)) >= 5             # skipped ids: empty users in between
        assert a.max() < F.RUN_ANIME and (len(np.unique(r)) == 11) == grid
    # over the four leads every run starts at every place of a lane's four rows
    assert sorted({int(F.run_starts(k)[5] % 4) for k in F.RUN_LEADS}) == [0, 1, 2, 3]


@pytest.mark.parametrize("n_anime", F.FUSE_ANIME)
def test_fuse_tables_set_the_last_bit_and_the_last_word(n_anime):
    assert F.FUSE_ANIME == (98303, 98304, 98305)
    ww = (n_anime + 31) // 32
    assert ww == {98303: 3072, 98304: 3072, 98305: 3073}[n_anime] and (ww * 16 <= 48 * 1024) == (ww <= F.FUSE_WORDS)
    u, a, r = F.fuse_table(n_anime)
    cnt = np.bincount(u, minlength=F.FUSE_USERS)
    assert len(cnt) == F.FUSE_USERS and cnt.max() == 40 and (cnt == 0).any() and _descents(u) == []
    assert a.min() >= 0 and a.max() == n_anime - 1
    _, bits = F.favourites(u, a, r, F.FUSE_USERS, n_anime)
    top = (bits[:, -1] >> np.uint32((n_anime - 1) & 31)) & 1
    assert top.sum() >= 40 and (bits[:, -1] != 0).sum() >= (40 if n_anime == 98305 else 80)
    past = np.uint32((0xFFFFFFFF << (n_anime & 31)) & 0xFFFFFFFF) if n_anime & 31 else np.uint32(0)
    assert not (bits[:, -1] & past).any()                                # no bit past the last anime


def test_workload_table_and_sample():
    u, a, r = F.workload_table()
    cnt = np.bincount(u, minlength=F.WORKLOAD_USERS)
    assert len(cnt) == 350_000 and cnt.min() == 0 and cnt.max() == 24 and 4.1e6 < len(u) < 4.5e6
    assert _descents(u) == [] and a.max() == F.WORKLOAD_ANIME - 1 == 1023 and len(np.unique(r)) == 11
    sample = F.workload_sample()
    assert 1990 <= len(sample) <= 2000 and len(np.unique(sample // F.TILE)) == 86


def test_error_table():
    for n_anime in (F.SCAN_ANIME, F.BREAK_UNFUSED_ANIME):
        u, a, r = F.error_table(n_anime)
        cnt = np.bincount(u, minlength=F.ERR_USERS)
        assert cnt[50] == 0 and cnt[0] >= 1 and cnt[-1] >= 1 and _descents(u) == [] and a.max() < n_anime


# ---------------------------------------------------------------- workspace size
def _al256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("n_users", [4096, 4097, 1024 * 4096 + 1])
def test_workspace_size_is_the_layout_it_documents(n_users):
    """cnt | ptr | cursor | csr_rating | 256 spare bytes | tile totals of the scan (csrc/anirec_recs.hip)."""
    from anime_recommendations_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    for n in (1, 33, 20_000):
        tiles = (n_users + 4095) // 4096
        want = _al256(4 * n_users) + 2 * _al256(8 * (n_users + 1)) + _al256(8 * n) + 256 + _al256(8 * tiles)
        assert int(lib.anirec_fav_workspace_bytes(n, n_users)) == want
    assert int(lib.anirec_fav_workspace_bytes(0, n_users)) == 0 and int(lib.anirec_fav_workspace_bytes(5, 0)) == 0
