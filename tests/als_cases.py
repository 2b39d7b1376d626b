"""The inputs the ALS tests share (tests/test_als_cpu.py measures the fp32 restatement on them, tests/test_als_gpu.py
holds the kernels to the fp64 one on the same): a 97-item frozen table, 40 rows of every list length at which the kernel
can go wrong, and the recorded distances that bound the kernel.

Lengths: 0, 1 and 2; each count of lane groups per pass (1024 / width = 32, 16, 8, 4 entries are in flight per pass at
widths 32, 64, 128, 256), one below and one past it; 96 (nearly every item) and 700 with repeats (many passes at every
width); the rest random.  The kernel has no other length-dependent path.
Scales: frozen rows of elements ~ 1 / sqrt(F) (row norm ~ 1), start rows ~ 0.3 / sqrt(F).  Excess: NULL (alpha for
every entry) and per entry (alpha times a weight in [0.25, 1]).
"""
import functools

import numpy as np

import als_restatement as R

N_ITEMS = 97
N_ROWS = 40
WIDTHS = (32, 64, 128, 256)
LENGTHS = (0, 1, 2, 4, 5, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65, 96, 700)
LONG_ROW = LENGTHS.index(700)
PAIRS = ((1.0, 0.01), (40.0, 0.1))           # (alpha, lambda)
# (pair, cg_steps): 8 steps at the first pair only — at (40, 0.1) the systems have condition numbers of 1e4 and more,
# where eight fp32 steps end 1e-2 from the fp64 ones and no tolerance could hold an implementation
STEP_CASES = [(p, s) for p in (0, 1) for s in (0, 1, 2, 3)] + [(0, 8)]
CASES = [(d, p, s, per) for d in WIDTHS for (p, s) in STEP_CASES for per in (False, True)]

# The tolerance of the GPU tests is 8 x the distance of the fp32 restatement (the kernel's documented order) from the
# fp64 one ON THE SAME CASE, for row elements and row_loss separately: the kernel's order may differ from the
# restatement's in association, not in kind (DESIGN.md 4.7's rule, the same margin).  Measured on the CPU and held there
# by tests/test_als_cpu.py: (width, pair, cg_steps, per-entry excess) -> (largest |x32 - x64|, largest |loss32 - loss64|)
# over the 40 rows.  Zero steps leave the rows bit for bit: their row distance is 0.
# The kernel's own distances (one MI355X run): its rows and losses are the fp32 restatement's bit for bit on every row of
# every case, so they are the recorded ones — at most 1.15e-5 on a row element, 2.11e-3 on a loss.
DEV = {
    (32, 0, 0, False): (0.0, 3.31e-5),
    (32, 0, 0, True): (0.0, 8.85e-5),
    (32, 0, 1, False): (2.69e-7, 1.99e-4),
    (32, 0, 1, True): (1.07e-6, 1.44e-5),
    (32, 0, 2, False): (5.62e-7, 4.85e-5),
    (32, 0, 2, True): (2.08e-6, 5.62e-5),
    (32, 0, 3, False): (6.41e-7, 2.91e-5),
    (32, 0, 3, True): (2.31e-6, 2.81e-5),
    (32, 1, 0, False): (0.0, 1.91e-3),
    (32, 1, 0, True): (0.0, 7.65e-4),
    (32, 1, 1, False): (3.82e-7, 1.48e-3),
    (32, 1, 1, True): (3.81e-7, 6.10e-4),
    (32, 1, 2, False): (9.27e-7, 1.45e-3),
    (32, 1, 2, True): (9.30e-7, 1.04e-3),
    (32, 1, 3, False): (1.97e-6, 1.62e-3),
    (32, 1, 3, True): (1.45e-6, 4.86e-4),
    (32, 0, 8, False): (7.82e-7, 5.40e-5),
    (32, 0, 8, True): (2.61e-6, 1.22e-5),
    (64, 0, 0, False): (0.0, 2.12e-4),
    (64, 0, 0, True): (0.0, 5.15e-5),
    (64, 0, 1, False): (3.08e-7, 6.33e-6),
    (64, 0, 1, True): (4.25e-7, 1.99e-5),
    (64, 0, 2, False): (6.95e-7, 2.45e-5),
    (64, 0, 2, True): (7.23e-7, 1.90e-5),
    (64, 0, 3, False): (1.05e-6, 2.82e-5),
    (64, 0, 3, True): (1.05e-6, 1.54e-5),
    (64, 1, 0, False): (0.0, 6.69e-4),
    (64, 1, 0, True): (0.0, 6.29e-4),
    (64, 1, 1, False): (4.41e-7, 1.15e-3),
    (64, 1, 1, True): (3.65e-7, 2.75e-4),
    (64, 1, 2, False): (1.28e-6, 2.80e-4),
    (64, 1, 2, True): (7.12e-7, 2.58e-4),
    (64, 1, 3, False): (5.91e-6, 9.72e-4),
    (64, 1, 3, True): (3.23e-6, 5.05e-4),
    (64, 0, 8, False): (2.10e-6, 1.69e-5),
    (64, 0, 8, True): (1.99e-6, 9.26e-6),
    (128, 0, 0, False): (0.0, 4.43e-5),
    (128, 0, 0, True): (0.0, 1.16e-4),
    (128, 0, 1, False): (3.40e-7, 1.14e-5),
    (128, 0, 1, True): (4.36e-7, 2.91e-5),
    (128, 0, 2, False): (9.99e-7, 4.14e-5),
    (128, 0, 2, True): (1.17e-6, 1.30e-4),
    (128, 0, 3, False): (1.57e-6, 1.28e-4),
    (128, 0, 3, True): (2.01e-6, 2.60e-5),
    (128, 1, 0, False): (0.0, 2.11e-3),
    (128, 1, 0, True): (0.0, 1.55e-3),
    (128, 1, 1, False): (5.10e-7, 1.86e-3),
    (128, 1, 1, True): (3.89e-7, 6.22e-4),
    (128, 1, 2, False): (8.88e-7, 1.15e-3),
    (128, 1, 2, True): (6.08e-7, 9.15e-5),
    (128, 1, 3, False): (1.15e-5, 9.22e-4),
    (128, 1, 3, True): (1.54e-6, 2.81e-4),
    (128, 0, 8, False): (7.25e-6, 1.74e-5),
    (128, 0, 8, True): (8.89e-6, 1.97e-4),
    (256, 0, 0, False): (0.0, 1.98e-4),
    (256, 0, 0, True): (0.0, 7.41e-5),
    (256, 0, 1, False): (6.65e-7, 4.11e-6),
    (256, 0, 1, True): (6.14e-7, 1.93e-4),
    (256, 0, 2, False): (1.92e-6, 4.24e-5),
    (256, 0, 2, True): (1.21e-6, 1.91e-4),
    (256, 0, 3, False): (3.63e-6, 2.92e-5),
    (256, 0, 3, True): (2.19e-6, 1.97e-4),
    (256, 1, 0, False): (0.0, 1.14e-3),
    (256, 1, 0, True): (0.0, 2.98e-4),
    (256, 1, 1, False): (4.52e-7, 8.67e-4),
    (256, 1, 1, True): (4.14e-7, 2.87e-4),
    (256, 1, 2, False): (9.76e-7, 8.69e-5),
    (256, 1, 2, True): (9.64e-7, 2.65e-4),
    (256, 1, 3, False): (7.16e-6, 2.25e-4),
    (256, 1, 3, True): (3.52e-6, 1.21e-4),
    (256, 0, 8, False): (1.13e-5, 4.49e-4),
    (256, 0, 8, True): (6.79e-6, 1.45e-4),
}
# the whole fit (FIT below, 2 sweeps): the largest |X32 - X64| element, the largest |Y32 - Y64| element and the largest
# relative distance of a half-sweep's loss
FIT_DEV = (1.27e-5, 1.48e-7, 1.14e-7)


def tolerances(case):
    r, l = DEV[case]
    return 8 * r, 8 * l


@functools.lru_cache(maxsize=None)
def table(dim):
    rng = np.random.default_rng(3000 + dim)
    Y = (rng.standard_normal((N_ITEMS, dim)) / np.sqrt(dim)).astype(np.float32)
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def rows(dim):
    """(offsets int64 [41], idx int32, weight fp32 in [0.25, 1], start fp32 [40, dim]): one row per LENGTHS entry, then
    random lengths in 0 .. 96; no repeats inside a list but in the 700-entry one"""
    rng = np.random.default_rng(4000 + dim)
    lens = list(LENGTHS) + [int(v) for v in rng.integers(0, N_ITEMS, N_ROWS - len(LENGTHS))]
    parts = [rng.integers(0, N_ITEMS, n) if n > N_ITEMS else rng.permutation(N_ITEMS)[:n] for n in lens]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate(parts).astype(np.int32)
    weight = (0.25 + 0.75 * rng.random(len(idx))).astype(np.float32)
    start = (rng.standard_normal((N_ROWS, dim)) * 0.3 / np.sqrt(dim)).astype(np.float32)
    for a in (offsets, idx, weight, start):
        a.setflags(write=False)
    return offsets, idx, weight, start


def case_inputs(case):
    """(Y, G fp32: the fp64 Gram rounded once, offsets, idx, excess | None, alpha, start, lambda, cg_steps)"""
    dim, pair, steps, per = case
    alpha, lam = PAIRS[pair]
    Y = table(dim)
    off, idx, w, start = rows(dim)
    ex = (np.float32(alpha) * w).astype(np.float32) if per else None
    return Y, R.gram64(Y).astype(np.float32), off, idx, ex, alpha, start, lam, steps


@functools.lru_cache(maxsize=None)
def reference(case, dtype_name="float64"):
    """the restatement of every row of a case: (X [40, dim], row_loss [40]); computed once and shared, never modified"""
    Y, G, off, idx, ex, alpha, start, lam, steps = case_inputs(case)
    X, loss = R.half_sweep(Y, G, off, idx, ex, alpha, start, lam, steps, dtype=getattr(np, dtype_name))
    X.setflags(write=False)
    loss.setflags(write=False)
    return X, loss


# ---- a whole fit: 30 users x 23 items, every user and item with at least one pair ------------------------------------
FIT = dict(n_users=30, n_items=23, factors=32, sweeps=2, cg_steps=3, alpha=1.0, reg=0.01, seed=5)
FIT_MIN_DECREASE = 1e-3         # a half-sweep's loss is compared with the one before only where the fp64 fit's relative
                                # decrease exceeds this, so rounding cannot decide the sign


@functools.lru_cache(maxsize=None)
def fit_pairs():
    rng = np.random.default_rng(77)
    like = rng.random((FIT["n_users"], FIT["n_items"])) < 0.25
    like[np.arange(FIT["n_users"]), rng.integers(0, FIT["n_items"], FIT["n_users"])] = True
    like[rng.integers(0, FIT["n_users"], FIT["n_items"]), np.arange(FIT["n_items"])] = True
    u, i = np.nonzero(like)
    perm = rng.permutation(len(u))                          # the pairs arrive in no order
    return u[perm].astype(np.int32), i[perm].astype(np.int32)


@functools.lru_cache(maxsize=None)
def fit_reference(dtype_name="float64"):
    u, i = fit_pairs()
    return R.fit(u, i, dtype=getattr(np, dtype_name), **FIT)


# ---- planted blocks: two disjoint taste groups ---------------------------------------------------------------------
# users 0 .. 39 like only items 0 .. 19, users 40 .. 79 only items 20 .. 39; block A's items are liked with probability
# 0.3, block B's with 0.6, so that popularity ranks every block-B item above block A's and a block-A user's held-out
# item lands behind the 20 items of the other block.  One liked pair per user is held out.
BLOCK = dict(n_users=80, n_items=40, factors=32, sweeps=6, cg_steps=2, alpha=1.0, reg=3.0, seed=1)


@functools.lru_cache(maxsize=None)
def block_pairs():
    """(train user, train item, held-out user, held-out item)"""
    rng = np.random.default_rng(11)
    like = np.zeros((80, 40), bool)
    like[:40, :20] = rng.random((40, 20)) < 0.3
    like[40:, 20:] = rng.random((40, 20)) < 0.6
    for u in range(80):                                     # every user likes at least three items of the block
        b = 0 if u < 40 else 20
        while like[u].sum() < 3:
            like[u, b + rng.integers(0, 20)] = True
    held = np.array([rng.choice(np.flatnonzero(like[u])) for u in range(80)])
    like[np.arange(80), held] = False
    u, i = np.nonzero(like)
    return u.astype(np.int32), i.astype(np.int32), np.arange(80, dtype=np.int32), held.astype(np.int32)


def mean_rank(scores, tu, ti, hu, hi):
    """the mean rank (0 = first) of the held-out items among the items their user has no training pair for; ties by
    ascending index"""
    seen = np.zeros(scores.shape, bool)
    seen[tu, ti] = True
    ranks = []
    for u, t in zip(hu, hi):
        s = scores[u]
        ahead = (~seen[u]) & ((s > s[t]) | ((s == s[t]) & (np.arange(len(s)) < t)))
        ahead[t] = False
        ranks.append(int(ahead.sum()))
    return float(np.mean(ranks))
