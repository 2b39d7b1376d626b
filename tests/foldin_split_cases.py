"""The inputs the tests of the split fold-in share (anirec_fold_in_split; tests/test_foldin_split_cpu.py measures the
fp32 restatement on them, tests/test_foldin_split_gpu.py holds the kernel to the fp64 one on the same): a 211-row
frozen table with one zero row and one fitted row per list length at which the chunking can go wrong — the chunk
edges 1024 and 2048, one before and one past, a ragged last chunk of 7 ratings (3079 = 3 * 1024 + 7), a five-chunk
list and the empty list.  The heads are foldin_cases.head_for's, so no rating comes near a point where its gradient
jumps (foldin_cases says why); the restatement asserts that on every step.

Step counts: 0, 1, 2, 8 and 50 — not the 100 of foldin_cases.  A long list has converged after 100 steps: its gradient
is rounding noise there, Adam's m / sqrt(v) turns the noise into full-size steps, and the float32 restatement ends
3.1e-5 (the 1023-rating list at width 256) to 1.7e-4 (the 5000-rating list under mean_squared_error + tanh) from the
float64 one, against 1.2e-6 on any row up to 50 steps.  No tolerance can hold an implementation there, so the parity
tests stop at 50 steps, where the float32 restatement stays inside foldin_cases.ROW_DEV / LOSS_DEV (held by
tests/test_foldin_split_cpu.py); the 100-step path is covered exactly instead: a list of at most 1024 ratings gives
the bits of anirec_fold_in, which foldin_cases holds at 100 steps.
"""
import functools

import numpy as np

import foldin_cases as K
import foldin_restatement as F

CHUNK = 1024                     # ANIREC_FOLD_CHUNK
N_TABLE = 211
ZERO_ROW = 13                    # a table row of zeros: normalises to zeros, contributes no gradient
LENGTHS = (0, 1, 1023, 1024, 1025, 2048, 2049, 3079, 5000)
STEPS = (0, 1, 2, 8, 50)
LR, L2 = K.LR, K.L2
CASES = [(d, "binary_crossentropy", "sigmoid") for d in K.WIDTHS] + \
        [(64, "huber", "linear"), (128, "mean_squared_error", "tanh"), (32, "mean_absolute_error", "relu"),
         (128, "log_cosh", "softplus")]


def alphas(steps=max(STEPS), lr=LR):
    return K.alphas(steps, lr)


@functools.lru_cache(maxsize=None)
def table(dim):
    rng = np.random.default_rng(3000 + dim)
    T = (rng.standard_normal((N_TABLE, dim)) * 0.05).astype(np.float32)
    T[ZERO_ROW] = 0
    return T


@functools.lru_cache(maxsize=None)
def lists(dim, binary_ratings=False):
    """(offsets int64, idx int32, rating fp32, init fp32 [n_new, dim]) of one fitted row per LENGTHS entry: indices drawn
    with replacement, ratings k / 10 (0 or 1 with ``binary_ratings``), the one-rating list rates 0.9 (out of the heads'
    reach: foldin_cases, Conditioning), start rows at the table's 0.05 scale.  The 1025-rating list meets the zero row
    twice: in its first chunk and as the only rating of its second."""
    rng = np.random.default_rng(3000 + dim)
    rng.standard_normal((N_TABLE, dim))                  # the table's draws
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    n = int(offsets[-1])
    idx = rng.integers(0, N_TABLE, n).astype(np.int32)
    j = LENGTHS.index(1025)
    idx[offsets[j] + 3] = idx[offsets[j] + 1024] = ZERO_ROW
    t = (rng.integers(0, 11, n) / 10.0).astype(np.float32)
    t[offsets[LENGTHS.index(1)]] = 0.9
    if binary_ratings:
        t = (t >= 0.7).astype(np.float32)
    init = (rng.standard_normal((len(LENGTHS), dim)) * 0.05).astype(np.float32)
    return offsets, idx, t, init


def case_inputs(dim, loss, act):
    off, idx, t, init = lists(dim, binary_ratings=(loss == "mean_absolute_error"))
    return table(dim), K.head_for(act, dim), off, idx, t, init


@functools.lru_cache(maxsize=None)
def reference(dim, loss, act, dtype_name="float64"):
    """the restatement of every row of a case after each of STEPS: {steps: (rows [n_new, dim], loss [n_new])};
    computed once per case and shared, never modified"""
    T, head, off, idx, t, init = case_inputs(dim, loss, act)
    res = F.fold_in_many(T, head, off, idx, t, init, alphas(), l2=L2, loss=loss, act=act,
                         dtype=getattr(np, dtype_name), snapshots=STEPS)
    out = {}
    for s in STEPS:
        rows = np.stack([r["snap"][s][0] for r in res])
        ls = np.array([r["snap"][s][1] for r in res])
        rows.setflags(write=False)
        ls.setflags(write=False)
        out[s] = (rows, ls)
    return out
