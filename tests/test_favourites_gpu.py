"""``anirec_user_favourites`` against NumPy where its eight launches change path: more than one tile of the row-pointer
scan (and more than one wave, more than one round, of its spine), a table grouped by user except for ONE row, runs of
equal users of every length and offset in the run-chained histogram, the widest bit row that is still built in LDS and
the first one that is not, ids out of range, and no rating at all.

Every comparison is exact: thresholds as uint64 after ``+ 0.0`` (tests/test_recs_gpu.py says why), NaN where the oracle
has NaN, the whole bit matrix word for word.  The oracle is ``oracle/recs_oracle.favourites``; where that cannot be run
(350 000 users) it is the restatement of tests/favourites_restatement.py, which tests/test_favourites_cpu.py holds to the
oracle bit for bit, plus the oracle itself on a sample.  The tables come from that module too, and the CPU file checks
on each of them the property its test here relies on.
"""

import numpy as np
import pytest
import torch

import favourites_restatement as F
from oracle import recs_oracle as orc

pytestmark = pytest.mark.gpu


def _cuda(x):
    return torch.as_tensor(x).cuda()


def _run(table, n_users, n_anime, pct=80.0):
    """(thr, fav) as the wrapper returns them, on the device."""
    from anime_recommendations_amd import recs
    u, a, r = table
    fav, thr = recs.user_favourites(_cuda(u), _cuda(a), _cuda(r), n_users, n_anime, pct)
    assert fav.dtype == torch.int32 and tuple(fav.shape) == (n_users, (n_anime + 31) // 32)
    assert thr.dtype == torch.float64 and tuple(thr.shape) == (n_users,)
    return thr, fav


def _same(got, want, what):
    """Thresholds and bit words, both whole, against (thr float64, bits uint32)."""
    thr, bits = got[0].cpu().numpy(), got[1].cpu().numpy().view(np.uint32)
    thr_w, bits_w = want
    bad_t = np.nonzero(F.canon(thr) != F.canon(thr_w))[0]
    bad_b = np.nonzero((bits != bits_w).any(axis=1))[0]
    assert len(bad_t) == 0 and len(bad_b) == 0, \
        "%s: %d thresholds differ (first at user %s), %d bit rows differ (first at user %s)" % (
            what, len(bad_t), bad_t[:1].tolist(), len(bad_b), bad_b[:1].tolist())


def _oracle(table, n_users, n_anime, pct=80):
    u, a, r = table
    thr, fav = orc.favourites(u, a, r, n_users, pct)
    return thr, F.pack_sets(fav, n_anime)


def _orders(table):
    """The table grouped by user and shuffled."""
    return (("grouped", table), ("shuffled", F.shuffled(table, 5)))


# ---------------------------------------------------------------- 1, 2, 6: the scan over more than one tile
@pytest.mark.parametrize("n_users", F.SCAN_SMALL_USERS)
def test_scan_over_one_to_three_tiles(n_users):
    """One tile less one count, one tile, one tile and one count, two tiles and one count: every user has ratings, so
    every row pointer past the first tile carries that tile's base."""
    table = F.scan_small_table(n_users)
    want = _oracle(table, n_users, F.SCAN_ANIME)
    for name, t in _orders(table):
        _same(_run(t, n_users, F.SCAN_ANIME), want, (n_users, name))


@pytest.mark.parametrize("n_users", F.SCAN_LARGE_USERS)
def test_scan_spine_over_two_waves_and_two_rounds(n_users):
    """65 tiles: tile 64 is the first of the spine's second wave.  1 025 tiles: tile 1 024 is the first of its second
    round of 1 024.  About 3 000 users have ratings, the ends of the tiles around those edges among them: they are held
    to the oracle (run on them alone); every other user must come back NaN with an empty bit row, checked on the
    device."""
    table = F.scan_large_table(n_users)
    ids, thr_o, bits_o = F.subset_oracle(table, F.scan_large_users(n_users), F.SCAN_ANIME)
    rows = _cuda(ids)
    empty = torch.ones(n_users, dtype=torch.bool, device="cuda")
    empty[rows] = False
    for name, t in _orders(table):
        thr, fav = _run(t, n_users, F.SCAN_ANIME)
        _same((thr[rows], fav[rows]), (thr_o, bits_o), (n_users, name))
        n_thr, n_bits = int((~torch.isnan(thr[empty])).sum()), int((fav[empty] != 0).any(dim=1).sum())
        assert n_thr == 0 and n_bits == 0, "%s: of the users without ratings %d have a threshold, %d a favourite" % (
            (n_users, name), n_thr, n_bits)
        del thr, fav


def test_the_workloads_user_count():
    """350 000 users (86 tiles, two waves of the spine) with 0 to 24 grid ratings each: everything against the
    restatement, 2 000 users across the tiles against the pandas oracle as well."""
    table = F.workload_table()
    want = F.favourites(*table, F.WORKLOAD_USERS, F.WORKLOAD_ANIME)
    ids, thr_o, bits_o = F.subset_oracle(table, F.workload_sample(), F.WORKLOAD_ANIME)
    assert np.array_equal(F.canon(want[0][ids]), F.canon(thr_o)) and np.array_equal(want[1][ids], bits_o)
    rows = _cuda(ids)
    for name, t in _orders(table):
        thr, fav = _run(t, F.WORKLOAD_USERS, F.WORKLOAD_ANIME)
        _same((thr, fav), want, name)
        _same((thr[rows], fav[rows]), (thr_o, bits_o), (name, "oracle sample"))
        del thr, fav


# ---------------------------------------------------------------- 3: one descent
@pytest.mark.parametrize("tail", F.BREAK_TAILS)
def test_one_row_out_of_place(tail):
    """A table grouped by user but for row p, which belongs to user 0: the order test has that one descent to find, at a
    quad, lane-0, wave, unroll and workgroup edge and in the last rows of an n % 4 tail.  Missed, the table is read in
    place with user 0's count in front of it and every later segment is one row off.  At 40 anime the bit rows come
    from the fused path if the table passes for grouped; at 98 305 anime there is no fused path.  Then the same
    descents made the other way round, by giving row p - 1 to the last user: row p and its quad are then as in the
    grouped table, and only the comparison with the row on its left can find the descent."""
    for n_anime, positions in ((F.SCAN_ANIME, F.break_positions(tail)),
                               (F.BREAK_UNFUSED_ANIME, F.break_unfused_positions(tail))):
        for p in (None,) + tuple(positions):
            table = F.break_table(tail, n_anime, p)
            _same(_run(table, F.BREAK_USERS, n_anime), _oracle(table, F.BREAK_USERS, n_anime), (tail, n_anime, p))
    for p in F.break_high_positions(tail):
        table = F.break_table(tail, F.SCAN_ANIME, p, high=True)
        _same(_run(table, F.BREAK_USERS, F.SCAN_ANIME), _oracle(table, F.BREAK_USERS, F.SCAN_ANIME), (tail, "high", p))


# ---------------------------------------------------------------- 4: run shapes
@pytest.mark.parametrize("grid", [True, False], ids=["grid", "continuous"])
@pytest.mark.parametrize("lead", F.RUN_LEADS)
def test_runs_of_every_length_at_every_offset(lead, grid):
    """The run-chained histogram: runs shorter than a lane's four rows, a wave's 256, an unroll step's 1 024 and a
    workgroup's 4 096 rows and longer, runs of one row between long ones, each starting at row 0, 1, 2 or 3 of a lane
    depending on ``lead``; user ids left out in between."""
    table, n_users = F.run_table(lead, grid)
    for pct in (80, 37.5):
        want = _oracle(table, n_users, F.RUN_ANIME, pct)
        for name, t in _orders(table):
            _same(_run(t, n_users, F.RUN_ANIME, pct), want, (lead, grid, pct, name))


# ---------------------------------------------------------------- 5: the fuse boundary
@pytest.mark.parametrize("n_anime", F.FUSE_ANIME)
def test_bit_rows_at_the_fuse_boundary(n_anime):
    """3 072 words is the widest row built in LDS (98 303 anime: its last bit unused; 98 304: all used); 3 073 words
    (98 305 anime) go through the zero-fill and the atomic pass.  The last anime and the last word are favourites of
    many users."""
    table = F.fuse_table(n_anime)
    want = _oracle(table, F.FUSE_USERS, n_anime)
    for name, t in _orders(table):
        _same(_run(t, F.FUSE_USERS, n_anime), want, (n_anime, name))


# ---------------------------------------------------------------- 7: the error flag
def _bad_user_end(t, n_anime):
    t[0][-1] = F.ERR_USERS


def _bad_user_start(t, n_anime):
    t[0][0] = -1


def _bad_user_shuffled(t, n_anime):
    t[0][len(t[0]) // 3] = F.ERR_USERS


def _bad_anime(t, n_anime):
    t[1][len(t[1]) // 3] = n_anime


@pytest.mark.parametrize("n_anime,shuffle,spoil", [
    (F.SCAN_ANIME, False, _bad_user_end), (F.SCAN_ANIME, False, _bad_user_start), (F.SCAN_ANIME, True, _bad_user_shuffled),
    (F.SCAN_ANIME, False, _bad_anime), (F.BREAK_UNFUSED_ANIME, False, _bad_anime), (F.SCAN_ANIME, True, _bad_anime)],
    ids=["user-end-grouped", "user-start-grouped", "user-shuffled", "anime-grouped-fused", "anime-grouped-unfused",
         "anime-shuffled"])
def test_an_id_out_of_range_raises_and_leaves_nothing_behind(n_anime, shuffle, spoil):
    """A user id out of range is left out of the counts (k_rec_count), skipped by the scatter and by the bit pass, so
    every segment ends inside the table; an anime id out of range is skipped where the bit is set.  The wrapper raises
    the ValueError of ``ops._finish`` (the one flag convention of the wrapper layer), and the next call, with the id
    repaired, is the oracle's answer."""
    table = F.error_table(n_anime)
    if shuffle:
        table = F.shuffled(table, 9)
    spoilt = tuple(c.copy() for c in table)
    spoil(spoilt, n_anime)
    assert sum(int((x != y).sum()) for x, y in zip(spoilt, table)) == 1
    with pytest.raises(ValueError, match="out of range"):
        _run(spoilt, F.ERR_USERS, n_anime)
    _same(_run(table, F.ERR_USERS, n_anime), _oracle(table, F.ERR_USERS, n_anime), "repaired")


# ---------------------------------------------------------------- 8: no rating
def test_an_empty_table_is_answered_without_the_library(monkeypatch):
    from anime_recommendations_amd import recs

    def no_call(*args):
        raise AssertionError("an empty table must not reach the library: %s" % (args[0],))
    monkeypatch.setattr(recs, "_call", no_call)
    none = np.zeros(0, np.int32)
    want = _oracle((none, none, np.zeros(0)), 70, 33)
    assert np.isnan(want[0]).all() and not want[1].any()
    got = _run((none, none, np.zeros(0)), 70, 33)
    assert got[0].is_cuda and got[1].is_cuda
    _same(got, want, "empty")
