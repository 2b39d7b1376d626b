"""Shared cases of the EASE tests (tests/test_ease_cpu.py, tests/test_ease_gpu.py): seeded, small, built once."""
import functools

import numpy as np

import ease_restatement as R
from cooc_restatement import pack_bits


def random_bits(n, n_users, seed, rate=0.15):
    """(liked-by bit rows uint32 [n, ceil(n_users/32)], the bool matrix)"""
    B = np.random.default_rng(seed).random((n, n_users)) < rate
    return pack_bits(B), B


def gram_case(n, reg, seed=0, n_users=None):
    """A = B B^T + reg I over 2 n users (the GPU accuracy cases)"""
    n_users = 2 * n if n_users is None else n_users
    bits, _ = random_bits(n, max(1, n_users), 1000 + 7 * n + seed)
    return R.gram_matrix(bits, max(1, n_users), reg)


def residual_bound(A):
    """(8 x the larger of a LAPACK inverse's residual and n 2^-52, that residual): the project's ALS rule, the factor
    absorbs another summation order, not another algorithm"""
    ref = R.residual(A, np.linalg.inv(A))
    return 8.0 * max(ref, len(A) * 2.0 ** -52), ref


@functools.lru_cache(maxsize=None)
def planted(seed=5, n_items=240, n_blocks=6, n_users=1500):
    """The planted blocks: every user belongs to one block of items and likes item j of it with rate
    0.02 + 0.25 u_j^2 (u_j uniform per item), an item of another block with 0.15 x that.  One liked pair of every user
    with at least 3 is held out.  Returns a dict: B_train bool [n_items, n_users], the training pairs (user, item), the
    held-out (user, item) arrays, n_items, n_users."""
    rng = np.random.default_rng(seed)
    block = np.arange(n_items) * n_blocks // n_items
    rate = 0.02 + 0.25 * rng.random(n_items) ** 2
    home = rng.integers(0, n_blocks, n_users)
    p = np.where(block[:, None] == home[None, :], rate[:, None], 0.15 * rate[:, None])
    B = rng.random((n_items, n_users)) < p
    held_u, held_i = [], []
    for u in range(n_users):
        mine = np.flatnonzero(B[:, u])
        if len(mine) >= 3:
            i = int(rng.choice(mine))
            B[i, u] = False
            held_u.append(u)
            held_i.append(i)
    items, users = np.nonzero(B)
    return dict(B=B, user=users.astype(np.int32), item=items.astype(np.int32), held_user=np.asarray(held_u, np.int64),
                held_item=np.asarray(held_i, np.int64), n_items=n_items, n_users=n_users)


def planted_histories(case):
    """(offsets int32 [n_held + 1], hist_idx int32): the training items of every held-out pair's user, in item order"""
    B = case["B"]
    lists = [np.flatnonzero(B[:, u]).astype(np.int32) for u in case["held_user"]]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return off, np.concatenate(lists).astype(np.int32)


def hit_rate(rank, k=10):
    return float(np.mean(np.asarray(rank) < k))


def popularity_hit_rate(case, k=10):
    B = case["B"]
    pop = B.sum(1).astype(np.float32)
    seen = B[:, case["held_user"]].T
    rank = R.ranks(np.broadcast_to(pop, seen.shape), seen, np.arange(len(seen)), case["held_item"])
    return hit_rate(rank, k)


def score_lists(n, n_lists, seed, long_len, weights="positive"):
    """History lists over n items: empty, one entry, a repeated item, one of ``long_len`` entries, then random ones of
    up to 20.  ``weights``: None, "positive" or "signed" (multiples of 1/8 up to 2).  Returns (offsets int32, hist_idx
    int32, hist_w fp32 | None)."""
    rng = np.random.default_rng(seed)
    hists = [[], [n - 1], [0, 0, n // 2, 0], rng.integers(0, n, long_len)]
    hists += [rng.integers(0, n, rng.integers(0, 21)) for _ in range(n_lists - len(hists))]
    hists = [np.asarray(h, np.int32) for h in hists[:n_lists]]
    off = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int32)
    hist = np.concatenate(hists).astype(np.int32)
    if weights is None:
        return off, hist, None
    w = rng.integers(1, 17, len(hist)) / 8.0
    if weights == "signed":
        w = w * rng.choice([-1.0, 1.0, 0.0], len(hist), p=[0.4, 0.5, 0.1])
    return off, hist, w.astype(np.float32)
