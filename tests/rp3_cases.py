"""Shared cases of the RP3 tests (tests/test_rp3_cpu.py, tests/test_rp3_gpu.py): seeded, small, built once."""
import functools

import numpy as np

from cooc_restatement import pack_bits

MAX_Q = 16383
LIMB_VALUES = (0, 1, 127, 128, 129, 16383)      # both sides of the 7-bit limb carry, and the two ends of the range


@functools.lru_cache(maxsize=None)
def bits_case(n_items, n_users, seed=0, rate=0.35):
    """(liked-by bit rows uint32 [n_items, ceil(n_users/32)] with GARBAGE in the bits past n_users, the bool matrix)"""
    rng = np.random.default_rng(9000 + 131 * n_items + 7 * n_users + seed)
    B = rng.random((n_items, n_users)) < rate
    B[:, 0] |= rng.random(n_items) < 0.5                     # (one user alone still gives co-occurrences)
    bits = pack_bits(B)
    if n_users & 31:
        junk = rng.integers(0, 1 << 32, n_items, dtype=np.uint64).astype(np.uint32)
        bits[:, -1] |= junk & ~np.uint32((1 << (n_users & 31)) - 1)
    return bits, B


def user_weights(kind, n_users, seed=0):
    """int32 [n_users]: "ones"; "limbs" (LIMB_VALUES mixed); "distinct" (a different value per user while they last)"""
    rng = np.random.default_rng(77 + n_users + seed)
    if kind == "ones":
        return np.ones(n_users, np.int32)
    if kind == "limbs":
        return rng.choice(np.asarray(LIMB_VALUES), n_users).astype(np.int32)
    assert kind == "distinct"
    return (1 + (np.arange(n_users, dtype=np.int64) * 7919 + 13 * seed) % MAX_Q).astype(np.int32)


def scales(n_items):
    """(row_scale, col_scale) fp64: non-trivial, different from each other, nowhere symmetric in (i, j)"""
    i = np.arange(n_items, dtype=np.float64)
    return (i + 1.37) ** -0.7, (2.0 * i + 3.11) ** -0.31


def queries(n_items, nq, seed=0):
    """int32 [nq]: a shuffled draw of the items that holds repeats whenever nq > 1"""
    rng = np.random.default_rng(5 + 3 * n_items + nq + seed)
    q = rng.permutation(n_items)[:nq]
    q = np.concatenate([q, rng.integers(0, n_items, nq - len(q))])
    if nq > 1:
        q[-1] = q[0]
    return rng.permutation(q).astype(np.int32)


def nine_items():
    """The 9-item, 40-user case of the literal loops: (B bool, user_q, queries, row_scale, col_scale)"""
    _, B = bits_case(9, 40, 3)
    row, col = scales(9)
    return B, user_weights("limbs", 40, 1), queries(9, 7, 2), row, col
