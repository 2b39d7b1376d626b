"""TEST INFRASTRUCTURE — vectorised NumPy restatement of ``oracle/recs_oracle.favourites`` and the rating tables of
tests/test_favourites_gpu.py.  Only tests/ may import this module.

``recs_oracle.favourites`` walks a pandas groupby and keeps one Python set per user: fine for a few thousand users,
unusable at the workload's 350 000 or at the 4 M of the scan tests.  ``favourites`` below states the same thing with
array operations (tests/test_favourites_cpu.py holds it to the oracle bit for bit), and ``dense_users`` maps the few
non-empty users of a huge range onto 0 .. m-1 so that the oracle itself can be run on them.

The table builders are here, not in the GPU file, because each one promises a property its test relies on (one descent
at the stated row, the stated run starts, thresholds that tell neighbouring users apart) and the CPU file checks that
promise on every table the GPU file uses.
"""
import numpy as np

from oracle import recs_oracle

TILE = 4096                     # counts per tile of the exclusive scan (kRsTile)
FUSE_WORDS = 3072               # the widest bit row k_rec_percentile builds in LDS (wwords * 16 <= 48 KiB)
PERCENTILES = (0, 37.5, 50, 80, 99.5, 100)


# ---------------------------------------------------------------- the restatement
def favourites(user_idx, anime_idx, rating, n_users, n_anime, pct=80):
    """(thr float64 [n_users], NaN for a user without ratings; bits uint32 [n_users, ceil(n_anime/32)]).
    thr[u] = np.percentile(ratings of u, pct) with the default 'linear' method; bit a of row u is set iff u rated a
    at or above thr[u]."""
    u = np.asarray(user_idx, np.int64)
    a = np.asarray(anime_idx, np.int64)
    r = np.asarray(rating, np.float64)
    ww = (int(n_anime) + 31) // 32
    thr = np.full(n_users, np.nan)
    bits = np.zeros((n_users, ww), np.uint32)
    if len(u) == 0:
        return thr, bits
    rs = r[np.lexsort((r, u))]                                   # by user, by rating inside a user
    cnt = np.bincount(u, minlength=n_users)
    start = np.cumsum(cnt) - cnt
    ne = np.nonzero(cnt)[0]
    n = cnt[ne]
    pos = (pct / 100) * (n - 1)                                  # numpy: quantile * (n - 1), in float64
    lo = np.floor(pos)
    t = pos - lo
    lo = lo.astype(np.int64)
    x_lo = rs[start[ne] + lo]
    x_hi = rs[start[ne] + np.minimum(lo + 1, n - 1)]
    diff = x_hi - x_lo                                           # numpy.lib._function_base_impl._lerp
    out = x_lo + diff * t
    out = np.where(t >= 0.5, x_hi - diff * (1 - t), out)
    thr[ne] = np.where(t == 0, x_lo, out)
    f = r >= thr[u]
    key = u[f] * ww + (a[f] >> 5)                                # one word of the matrix per key
    bit = np.uint32(1) << (a[f] & 31).astype(np.uint32)
    order = np.argsort(key, kind="stable")
    key, bit = key[order], bit[order]
    if len(key):
        first = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0]
        bits.reshape(-1)[key[first]] = np.bitwise_or.reduceat(bit, first)
    return thr, bits


def dense_users(user_idx):
    """(ids, dense): the sorted distinct user ids of the column, and the column with each id replaced by its place
    in ``ids``.  ``recs_oracle.favourites(dense, ..., len(ids))`` is then the oracle of those users alone."""
    ids, dense = np.unique(np.asarray(user_idx, np.int64), return_inverse=True)
    return ids, dense.reshape(-1).astype(np.int32)


def pack_sets(fav, n_anime):
    """The oracle's list of sets as bit words uint32 [len(fav), ceil(n_anime/32)]."""
    bits = np.zeros((len(fav), (n_anime + 31) // 32), np.uint32)
    for u, s in enumerate(fav):
        for x in s:
            bits[u, x >> 5] |= np.uint32(1 << (x & 31))
    return bits


def canon(thr):
    """Thresholds as the bits compared: ``+ 0.0`` first (the sign of a zero is an accident of numpy's partition), and
    every NaN as one pattern."""
    thr = np.asarray(thr, np.float64) + 0.0
    return np.where(np.isnan(thr), np.nan, thr).view(np.uint64)


# ---------------------------------------------------------------- tables
def _table(u, a, r):
    return (np.ascontiguousarray(u, np.int32), np.ascontiguousarray(a, np.int32), np.ascontiguousarray(r, np.float64))


def shuffled(table, seed):
    p = np.random.default_rng(seed).permutation(len(table[0]))
    return tuple(c[p] for c in table)


def _few_ratings(rng, users, n_anime, lo=1, hi=12, grid=False):
    """Grouped table in which each of ``users`` (ascending) has lo .. hi ratings of distinct anime."""
    sizes = rng.integers(lo, hi + 1, len(users))
    u = np.repeat(users, sizes)
    j = np.arange(len(u)) - np.repeat(np.cumsum(sizes) - sizes, sizes)      # 0, 1, .. inside a user
    a = (np.repeat(rng.integers(0, n_anime, len(users)), sizes) + j) % n_anime
    r = rng.integers(0, 11, len(u)) / 10 if grid else rng.random(len(u))
    return _table(u, a, r)


SCAN_SMALL_USERS = (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
SCAN_LARGE_USERS = (64 * TILE + 1, 1024 * TILE + 1)             # 65 tiles: two waves of the spine; 1 025: two rounds
SCAN_ANIME = 40


def scan_small_table(n_users):
    """Every user has 1 to 12 continuous ratings: each count of each tile matters to the row pointers after it."""
    return _few_ratings(np.random.default_rng(n_users), np.arange(n_users), SCAN_ANIME)


def scan_large_users(n_users):
    """The non-empty users of the large scan tables: both ends of the tiles around the spine's wave and round edges,
    the last user, and about 3 000 others."""
    n_tiles = (n_users + TILE - 1) // TILE
    edge = [x for t in (0, 1, 2, 62, 63, 64, 1022, 1023, 1024) if t < n_tiles
            for x in (t * TILE, min(t * TILE + TILE - 1, n_users - 1))]
    rnd = np.random.default_rng(n_users).integers(0, n_users, 3000)
    return np.unique(np.r_[edge, n_users - 1, rnd])


def scan_large_table(n_users):
    return _few_ratings(np.random.default_rng(n_users + 1), scan_large_users(n_users), SCAN_ANIME)


BREAK_USERS = 61
BREAK_TAILS = (0, 1, 2, 3)
BREAK_UNFUSED_ANIME = 32 * FUSE_WORDS + 1


def break_rows(tail):
    return 3 * TILE + tail


def break_positions(tail):
    n = break_rows(tail)
    return (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, n - 2, n - 1)


def break_unfused_positions(tail):
    return (256, 1024, 4096, break_rows(tail) - 1)


def break_high_positions(tail):
    return break_positions(tail)[:-2]


def break_table(tail, n_anime, p=None, high=False):
    """3 * 4096 + tail rows grouped by user: users 1 .. 60 with about 200 continuous ratings each, user 0 with none.
    With ``p``, row p is handed to user 0: the row before it belongs to a user >= 1 and so does the row after, so the
    table's one descent is at p.  With ``high`` it is row p - 1 that changes hands, to the last user: the descent is
    again at p alone (p before the last user's own rows), now with the larger id on its left and nothing unusual in
    row p itself.  No user begins in rows 1 .. 3 of a wave's 256: the first quad of every wave is of one user, so it
    says nothing about the order unless it is compared with the row before it."""
    n = break_rows(tail)
    rng = np.random.default_rng(100 + tail)
    cuts = np.arange(1, BREAK_USERS - 1) * n // (BREAK_USERS - 1) + rng.integers(-40, 41, BREAK_USERS - 2)
    cuts += np.where((cuts % 256 >= 1) & (cuts % 256 <= 3), 4, 0)
    u = np.searchsorted(cuts, np.arange(n), side="right") + 1
    a = rng.integers(0, n_anime, n)
    a[::97] = n_anime - 1 - (np.arange(len(a[::97])) % min(n_anime, 33))    # the last word is in use
    r = rng.random(n)
    if p is not None:
        u[p - 1 if high else p] = BREAK_USERS - 1 if high else 0
    return _table(u, a, r)


RUN_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1, 1, 1, 1023, 1024, 1025, 2, 4093, 4096, 4099, 3, 20000, 1,
               70000, 1, 1)
RUN_LEADS = (0, 1, 2, 3)
RUN_ANIME = 3000


def run_users(lead):
    """User ids of the run table: ``lead`` single-row users, then one user per run with every sixth id left out."""
    i = np.arange(len(RUN_LENGTHS))
    return np.r_[np.arange(lead), lead + i + i // 5]


def run_starts(lead):
    """The row at which each of RUN_LENGTHS begins."""
    return lead + np.cumsum((0,) + RUN_LENGTHS[:-1])


def run_table(lead, grid):
    """(table, n_users): one grouped table of the run lengths above, each run start shifted by ``lead`` rows."""
    rng = np.random.default_rng(200 + lead)
    users = run_users(lead)
    u = np.repeat(users, (1,) * lead + RUN_LENGTHS)
    a = rng.integers(0, RUN_ANIME, len(u))
    r = rng.integers(0, 11, len(u)) / 10 if grid else rng.random(len(u))
    return _table(u, a, r), int(users[-1]) + 2                  # the last user id is empty too


FUSE_ANIME = (32 * FUSE_WORDS - 1, 32 * FUSE_WORDS, 32 * FUSE_WORDS + 1)
FUSE_USERS = 300


def fuse_table(n_anime):
    """300 users with up to 40 continuous ratings in [0, 1).  Every seventh user rates anime n_anime - 1 with 2.0, the
    users after them some other anime of the last word: above every threshold, so those bits are favourites."""
    rng = np.random.default_rng(n_anime)
    sizes = rng.integers(0, 41, FUSE_USERS)
    sizes[::7] = np.maximum(sizes[::7], 1)
    sizes[1::7] = np.maximum(sizes[1::7], 1)
    u = np.repeat(np.arange(FUSE_USERS), sizes)
    a = rng.integers(0, n_anime, len(u))
    r = rng.random(len(u))
    first = (np.cumsum(sizes) - sizes)
    top = first[::7]
    a[top], r[top] = n_anime - 1, 2.0
    last_word = 32 * ((n_anime - 1) // 32)
    near = first[1::7]
    a[near], r[near] = last_word + np.arange(len(near)) % (n_anime - last_word), 2.0
    return _table(u, a, r)


WORKLOAD_USERS, WORKLOAD_ANIME = 350_000, 1024


def workload_table():
    """The benchmark's user count: 86 scan tiles, 0 to 24 grid ratings per user."""
    return _few_ratings(np.random.default_rng(350), np.arange(WORKLOAD_USERS), WORKLOAD_ANIME, 0, 24, grid=True)


def workload_sample():
    """2 000 users across the tiles, for the pandas oracle."""
    return np.unique(np.linspace(0, WORKLOAD_USERS - 1, 2000).astype(np.int64))


ERR_USERS = 100


def error_table(n_anime):
    """100 users with 1 to 30 continuous ratings each (user 50 has none), grouped."""
    users = np.delete(np.arange(ERR_USERS), 50)
    return _few_ratings(np.random.default_rng(7), users, n_anime, 1, 30)


def subset_oracle(table, users, n_anime, pct=80):
    """``recs_oracle.favourites`` on the rows of ``users`` only (through the dense range): (ids, thr, bits)."""
    u, a, r = table
    rows = np.isin(u, users)
    ids, dense = dense_users(u[rows])
    thr, fav = recs_oracle.favourites(dense, a[rows], r[rows], len(ids), pct)
    return ids, thr, pack_sets(fav, n_anime)
