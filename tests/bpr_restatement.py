"""NumPy restatement of the BPR matrix factorisation of include/anirec.h (anirec_bpr_sample / anirec_bpr_steps; DESIGN.md
4.27): the hashed sampler, the stated sigmoid, one step with its int64 sums, the whole fit, and the planted blocks the
ranking tests use.  A plain helper module, imported by the tests the way ``als_restatement`` is.  Every float operation
is on float32 arrays in the header's order, every sum across slots is an int64 sum, so the kernels must give these bits.
"""
import functools

import numpy as np

F32 = np.float32
WIDTHS = (32, 64, 128, 256)
MAX_TRIES = 16
ERR_INDEX, ERR_DIVERGED = 1, 2


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


L2E, C1, C2 = _bits(0x3FB8AA3B), _bits(0x3F317200), _bits(0x35BFBE8E)
POLY = (F32(1.0 / 720.0), F32(1.0 / 120.0), F32(1.0 / 24.0), F32(1.0 / 6.0), F32(0.5), F32(1.0), F32(1.0))
GOLD, KEYC = 0x9e3779b9, 0x85ebca6b
M32 = 0xFFFFFFFF


# ---- the sampler ------------------------------------------------------------------------------------------------------
def mix32(x):
    x = np.array(x, np.uint32, ndmin=1)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7feb352d)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846ca68b)
        x = x ^ (x >> np.uint32(16))
    return x


def slot_hash(seed, t, s):
    """h(t, s) for an array of slots"""
    step = mix32((int(seed) + GOLD * int(t)) & M32)
    with np.errstate(over="ignore"):
        return mix32(step ^ mix32(np.asarray(s, np.uint32) + np.uint32(KEYC)))


def draw(h, c):
    with np.errstate(over="ignore"):
        return mix32(h + np.uint32((GOLD * (int(c) + 1)) & M32))


def pick(r, n):
    return ((r.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def csr(user_idx, item_idx, n_users, n_items):
    """(offsets int64 [n_users + 1], idx int32 [nnz], pair_user int32 [nnz]) of the DISTINCT pairs, items ascending
    inside a row"""
    key = np.unique(np.asarray(user_idx, np.int64) * int(n_items) + np.asarray(item_idx, np.int64))
    pu, ix = (key // int(n_items)).astype(np.int32), (key % int(n_items)).astype(np.int32)
    off = np.zeros(int(n_users) + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(pu, minlength=int(n_users)))
    return off, ix, pu


def sample(off, idx, pair_user, n_items, batch, tries, seed, step0, n_steps):
    """int32 [n_steps, batch, 3]: (u, i, j), j = -1 for a dropped slot, (-1, -1, -1) for an index out of range"""
    n_users, nnz = len(off) - 1, len(idx)
    out = np.full((int(n_steps), int(batch), 3), -1, np.int32)
    idx, pair_user = np.asarray(idx, np.int64), np.asarray(pair_user, np.int64)
    # (row, item) of every entry as one key: membership in a row is membership of the key (rows ascending, no repeats)
    liked_keys = (np.repeat(np.arange(n_users, dtype=np.int64), np.diff(off)) << 32) | (idx & M32)
    for k in range(int(n_steps)):
        h = slot_hash(seed, int(step0) + k, np.arange(int(batch)))
        p = pick(draw(h, 0), nnz)
        u, i = pair_user[p], idx[p]
        ok = (u >= 0) & (u < n_users) & (i >= 0) & (i < n_items)
        us = np.where(ok, u, 0)
        j = np.full(int(batch), -1, np.int64)
        for c in range(1, int(tries) + 1):
            cand = pick(draw(h, c), n_items)
            liked = np.isin((us << 32) | cand, liked_keys)
            take = ok & (j < 0) & ~liked
            j[take] = cand[take]
        out[k, :, 0], out[k, :, 1], out[k, :, 2] = np.where(ok, u, -1), np.where(ok, i, -1), j
    return out


def in_row(off, idx, u, item):
    """whether ``item`` is in row ``u``, by the binary search the kernel makes (the literal form of ``sample``'s test)"""
    row = np.asarray(idx[off[u]:off[u + 1]])
    at = np.searchsorted(row, item)
    return bool(at < len(row) and row[at] == item)


# ---- the sigmoid ------------------------------------------------------------------------------------------------------
def sigmoid_neg(x):
    """g = 1 / (1 + e(x)) of the header for a float32 array"""
    x = np.asarray(x, F32)
    xc = np.fmin(np.fmax(x, F32(-30.0)), F32(30.0))
    kf = np.rint(xc * L2E)
    r = (xc - kf * C1) - kf * C2
    p = np.full_like(r, POLY[0])
    for c in POLY[1:]:
        p = p * r + c
    e = np.ldexp(p, kf.astype(np.int32))
    assert e.dtype == np.float32
    return F32(1.0) / (F32(1.0) + e)


def x_hat(x, d):
    """sum_k x[k] d[k] per row of float32 [n, F] arrays, in the header's order"""
    n, width = x.shape
    kg = width // 4
    a, b = x.reshape(n, kg, 4), d.reshape(n, kg, 4)
    v = ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]
    lanes, o = np.arange(kg), kg // 2
    while o >= 1:
        v = v + v[:, lanes ^ o]
        o //= 2
    return v[:, 0]


# ---- one step ---------------------------------------------------------------------------------------------------------
def _fixed(v):
    """(the int64 terms of float32 products, whether any broke the 2^20 guard)"""
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(v) <= F32(1048576.0))
    t = np.rint(np.where(bad, F32(0), v).astype(np.float64) * 1073741824.0).astype(np.int64)
    return t, bool(bad.any())


def step(X, Y, triples, lr, reg, bias, order=None):
    """(X', Y', (kept, dropped, positive), err bits) of one step over ``triples`` int32 [batch, 3]; ``order``: the order
    the slots are processed in (any permutation gives the same bits)"""
    X, Y = np.asarray(X, F32), np.asarray(Y, F32)
    trip = np.asarray(triples)
    if order is not None:
        trip = trip[np.asarray(order)]
    err = ERR_INDEX if (trip[:, 0] < 0).any() else 0
    live = trip[trip[:, 2] >= 0]
    u, i, j = live[:, 0], live[:, 1], live[:, 2]
    counts = (len(live), len(trip) - len(live))
    with np.errstate(over="ignore", invalid="ignore"):
        x = X[u]
        d = Y[i] - Y[j]
        xh = x_hat(x, d)
        g = sigmoid_neg(xh)[:, None]
        tu, bad_u = _fixed(g * d)
        ti, bad_i = _fixed(g * x)
    if bad_u or bad_i:
        err |= ERR_DIVERGED
    acc_x, acc_y = np.zeros(X.shape, np.int64), np.zeros(Y.shape, np.int64)
    np.add.at(acc_x, u, tu)
    np.add.at(acc_y, i, ti)
    np.add.at(acc_y, j, -ti)
    c_x = np.bincount(u, minlength=len(X))
    c_y = np.bincount(i, minlength=len(Y)) + np.bincount(j, minlength=len(Y))
    Xn, Yn = _apply(X, acc_x, c_x, lr, reg), _apply(Y, acc_y, c_y, lr, reg)
    if bias:
        Xn[:, -1] = X[:, -1]
    return Xn, Yn, counts + (int((xh > 0).sum()),), err


def _apply(T, acc, c, lr, reg):
    out = T.copy()
    rows = c > 0
    with np.errstate(over="ignore", invalid="ignore"):
        grad = (acc[rows].astype(np.float64) * 2.0 ** -30).astype(F32)
        rc = (F32(reg) * c[rows].astype(F32))[:, None]
        out[rows] = T[rows] + F32(lr) * (grad - rc * T[rows])
    return out


def steps(X, Y, off, idx, pair_user, batch, tries, seed, step0, n_steps, lr, reg, bias):
    """(X', Y', counts int64 [n_steps, 3], err bits) of anirec_bpr_steps"""
    X, Y = np.array(X, F32), np.array(Y, F32)
    counts, err = np.zeros((int(n_steps), 3), np.int64), 0
    for k in range(int(n_steps)):
        trip = sample(off, idx, pair_user, len(Y), batch, tries, seed, int(step0) + k, 1)[0]
        X, Y, counts[k], e = step(X, Y, trip, lr, reg, bias)
        err |= e
    return X, Y, counts, err


# ---- the whole fit ----------------------------------------------------------------------------------------------------
def start_tables(n_users, n_items, factors, bias, seed):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n_users, factors)) * 0.01).astype(F32)
    Y = (rng.standard_normal((n_items, factors)) * 0.01).astype(F32)
    if bias:
        X[:, -1], Y[:, -1] = 1.0, 0.0
    return X, Y


def fit(user_idx, item_idx, n_users, n_items, factors=64, epochs=30, batch=131072, lr=0.05, reg=0.01, tries=8, bias=True,
        seed=0):
    """(X, Y, per-epoch counts int64 [epochs, 3]) of recs.bpr_fit"""
    off, idx, pu = csr(user_idx, item_idx, n_users, n_items)
    X, Y = start_tables(n_users, n_items, factors, bias, seed)
    per = -(-len(idx) // int(batch))
    X, Y, counts, err = steps(X, Y, off, idx, pu, batch, tries, seed, 0, int(epochs) * per, lr, reg, int(bool(bias)))
    assert err == 0
    return X, Y, counts.reshape(int(epochs), per, 3).sum(axis=1)


# ---- planted blocks ---------------------------------------------------------------------------------------------------
BLOCK_SEEDS = (0, 1, 2)
BLOCK = dict(n_users=80, n_items=40, factors=32, epochs=30, batch=256, lr=0.05, reg=0.01, tries=8, bias=True, seed=0)


@functools.lru_cache(maxsize=None)
def block_pairs(data_seed):
    """(train user, train item, held-out user, held-out item): 80 users x 40 items, two taste blocks, half of the own
    block liked, 5 % noise across the blocks, one liked pair of the own block per user held out"""
    rng = np.random.default_rng(data_seed)
    like = np.zeros((80, 40), bool)
    like[:40, :20] = rng.random((40, 20)) < 0.5
    like[40:, 20:] = rng.random((40, 20)) < 0.5
    like[:40, 20:] = rng.random((40, 20)) < 0.05
    like[40:, :20] = rng.random((40, 20)) < 0.05
    held = np.zeros(80, np.int32)
    for u in range(80):
        b = 0 if u < 40 else 20
        while like[u, b:b + 20].sum() < 3:
            like[u, b + rng.integers(0, 20)] = True
        held[u] = b + rng.choice(np.flatnonzero(like[u, b:b + 20]))
    like[np.arange(80), held] = False
    u, i = np.nonzero(like)
    return u.astype(np.int32), i.astype(np.int32), np.arange(80, dtype=np.int32), held


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


@functools.lru_cache(maxsize=None)
def block_fit(data_seed):
    tu, ti, _, _ = block_pairs(data_seed)
    return fit(tu, ti, **BLOCK)
