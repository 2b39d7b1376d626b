"""The inputs the fold-in tests share (tests/test_foldin_cpu.py measures the fp32 restatement on them, tests/
test_foldin_gpu.py holds the kernel to the fp64 one on the same): a 97-anime table, new users of every list length at
which the kernel can go wrong, and heads under which no rating can reach a point where its gradient jumps.

Kinks.  c is a cosine, so y = c hs + hb lies in [hb - |hs|, hb + |hs|] whatever the row does.  HEAD keeps y in
[0.15, 0.85] (relu never at 0; sigmoid, tanh, linear, relu give p in (0.14, 0.86)), HEAD_SOFTPLUS keeps y in
[-1.3, -0.3] (p in (0.24, 0.56)): |p - t| < 1 (huber), p far from 1e-7 and 1 - 1e-7 (the clipped binary_crossentropy),
and for mean_absolute_error the ratings are 0 or 1, at least 0.14 from every reachable p.  By construction the nearest
jump is therefore 0.14 away (relu, mean_absolute_error, huber at |e| = 1: |e| <= 0.86) or further; the restatement
asserts on every step that none comes within foldin_restatement.KINK_MARGIN = 1e-4 — the distance that matters: far
above the row tolerance carried to p — so no case needs a skip.
Under those two heads |p - t| < 1 and p stays inside the binary_crossentropy clip, so huber's linear branch and the
clipped branch (gradient 0) would never run.  HEAD_FAR (the linear activation at width 64) keeps y = p in
[2.25, 2.95]: every rating sits on huber's linear branch (|e| >= 1.25) and beyond the clip (the row then moves by
the L2 term alone), again at least 0.25 from the jump.

Conditioning.  A list of one or two ratings that the head can reach exactly is fitted to zero data loss within a few
dozen steps; there the gradient is rounding noise, Adam's m / sqrt(v) turns it into full-size steps and the row
wanders on a chaotic orbit around the optimum: the float32 and float64 restatements of such a user end 4e-2 apart
after 100 steps (one rating of 0.6, width 128, sigmoid + log_cosh), against 1e-7 for every other user.  No tolerance
can hold an implementation there, so the users of one and two ratings rate 0, 0.1, 0.9 or 1 — outside the reach of
either head — and their fit runs into the boundary c = +-1 instead, which is well conditioned.
"""
import functools

import numpy as np

import foldin_restatement as F
from anime_recommendations_amd import schedule

N_ANIME = 97
ZERO_ANIME = 13                  # an anime row of zeros: normalises to zeros, contributes no gradient
WIDTHS = (32, 64, 128, 256)
# list lengths: the issue's, plus each count of lane groups per pass (256 / (width / 4) = 32, 16, 8, 4 ratings are in
# flight per pass at widths 32, 64, 128, 256) and one past it; the kernel has no other length-dependent path (no LDS
# stage of the rows)
LENGTHS = (0, 1, 2, 4, 5, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65, 700)
SHORT_USERS = 3                  # the users of 0, 1 and 2 ratings: their ratings are 0, 0.1, 0.9 or 1 (see above)
STEPS = (0, 1, 2, 8, 100)
LR, L2 = 0.01, 1e-4
# The tolerance of the GPU tests.  ROW_DEV / LOSS_DEV: the largest distance of the float32 restatement from the
# float64 one over every case, user and step count below, measured on the CPU and held there by tests/
# test_foldin_cpu.py — 3.14e-6 on a row element (width 128, mean_squared_error + tanh, the 5-rating user after ONE
# step: Adam's first step is lr g / (|g| + 3.2e-6), which magnifies the rounding of a gradient element of that size
# 3000-fold) and 1.81e-7 on the loss.  The kernel sums in another order (lane butterflies, per-group chains, groups in
# LDS order) and is allowed 8 x that.
ROW_DEV, LOSS_DEV = 3.14e-6, 1.81e-7        # measured: 3.1394e-6, 1.8056e-7
ROW_TOL, LOSS_TOL = 8 * ROW_DEV, 8 * LOSS_DEV
# inv = gamma / sqrt(mov_var + 1e-3) = 1: hs = w, hb = b + beta - mov_mean
HEAD = dict(w=0.35, b=0.3, gamma=0.8, beta=0.25, mov_mean=0.05, mov_var=0.639)
HEAD_SOFTPLUS = dict(w=0.5, b=-0.6, gamma=0.8, beta=-0.15, mov_mean=0.05, mov_var=0.639)
HEAD_FAR = dict(w=0.35, b=2.4, gamma=0.8, beta=0.25, mov_mean=0.05, mov_var=0.639)
FAR_DIM = 64                     # the width at which the linear activation runs under HEAD_FAR
# every width for the default head, widths 128 and 32 for every other loss x activation
HEAD_PAIRS = [(l, a) for l in F.LOSSES for a in F.ACTIVATIONS]
CASES = [(d, "binary_crossentropy", "sigmoid") for d in WIDTHS] + \
        [(d, l, a) for d in (128, 32) for (l, a) in HEAD_PAIRS if (l, a) != ("binary_crossentropy", "sigmoid")]
# the two cases under HEAD_FAR.  Their losses are 1.5 to 12 (a clipped binary_crossentropy term is 15.3 (1 - t)), where
# one float32 spacing is 1e-6: they carry their own measured distances, so that they do not widen the bound of the rest
FAR_CASES = [(FAR_DIM, "huber", "linear"), (FAR_DIM, "binary_crossentropy", "linear")]
FAR_ROW_DEV, FAR_LOSS_DEV = 9.48e-7, 1.15e-6         # measured: 9.480e-7 (huber, 8 steps), 1.148e-6 (the clipped loss)


def deviations(dim, loss, act):
    """(row, loss): the recorded float32-restatement distances that bound a case; the GPU tolerance is 8 x each"""
    return (FAR_ROW_DEV, FAR_LOSS_DEV) if (dim, loss, act) in FAR_CASES else (ROW_DEV, LOSS_DEV)


def tolerances(dim, loss, act):
    r, l = deviations(dim, loss, act)
    return 8 * r, 8 * l


def head_for(act, dim=128):
    if act == "linear" and dim == FAR_DIM:
        return dict(HEAD_FAR)
    return dict(HEAD_SOFTPLUS if act == "softplus" else HEAD)


def alphas(steps=max(STEPS), lr=LR):
    return schedule.adam_alphas(lr, 1, steps)


@functools.lru_cache(maxsize=None)
def table(dim):
    rng = np.random.default_rng(1000 + dim)
    A = (rng.standard_normal((N_ANIME, dim)) * 0.05).astype(np.float32)
    A[ZERO_ANIME] = 0
    return A


@functools.lru_cache(maxsize=None)
def users(dim, binary_ratings=False):
    """(offsets int64, anime_idx int32, rating fp32, init fp32 [n_new, dim]) of one user per LENGTHS entry; ratings k / 10
    (0 or 1 with ``binary_ratings``), anime drawn with replacement (repeats in the longer lists), start rows at the
    table's 0.05 scale"""
    rng = np.random.default_rng(2000 + dim)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    n = int(offsets[-1])
    idx = rng.integers(0, N_ANIME, n).astype(np.int32)
    idx[offsets[6]:offsets[6] + 2] = ZERO_ANIME          # the 8-rating user meets the zero row, twice
    t = (rng.integers(0, 11, n) / 10.0).astype(np.float32)
    short = offsets[SHORT_USERS]
    t[:short] = rng.choice(np.array([0.0, 0.1, 0.9, 1.0], np.float32), short)
    if binary_ratings:
        t = (t >= 0.7).astype(np.float32)
    init = (rng.standard_normal((len(LENGTHS), dim)) * 0.05).astype(np.float32)
    return offsets, idx, t, init


def case_inputs(dim, loss, act):
    off, idx, t, init = users(dim, binary_ratings=(loss == "mean_absolute_error"))
    return table(dim), head_for(act, dim), off, idx, t, init


@functools.lru_cache(maxsize=None)
def reference(dim, loss, act, dtype_name="float64"):
    """the restatement of every user of a case, rows and losses after each of STEPS: {steps: (rows [n_new, dim],
    loss [n_new])}; computed once per case and shared, never modified"""
    A, head, off, idx, t, init = case_inputs(dim, loss, act)
    res = F.fold_in_many(A, head, off, idx, t, init, alphas(), l2=L2, loss=loss, act=act,
                         dtype=getattr(np, dtype_name), snapshots=STEPS)
    out = {}
    for s in STEPS:
        rows = np.stack([r["snap"][s][0] for r in res])
        ls = np.array([r["snap"][s][1] for r in res])
        rows.setflags(write=False)
        ls.setflags(write=False)
        out[s] = (rows, ls)
    return out
