"""NumPy restatement of group recommendations (include/anirec.h, anirec_group_topk) from a grid of fp32 ratings — the
yardstick the GPU tests hold ops.group_topk to.  Every sum, divide and compare is fp32, in member order.  A plain
helper module, imported the way ``rank_restatement`` is."""
import numpy as np

from rank_restatement import score_key

MODES = ("mean", "min", "max")
NAN = np.float32(np.nan)


def aggregate(Pm, mode):
    """The aggregate of member ratings ``Pm`` fp32 [c, n] (c >= 1), member after member:
    mean  s = p_0; s = s + p_i; s / float32(c)
    min   a = p_0; p_i NaN -> a = p_i; else a not NaN and p_i < a -> a = p_i   (max: >)"""
    Pm = np.asarray(Pm, np.float32)
    a = Pm[0].copy()
    for p in Pm[1:]:
        if mode == "mean":
            with np.errstate(over="ignore", invalid="ignore"):
                a = (a + p).astype(np.float32)
        else:
            with np.errstate(invalid="ignore"):
                better = (p < a) if mode == "min" else (p > a)
            a = np.where(np.isnan(p), p, np.where(~np.isnan(a) & better, p, a)).astype(np.float32)
    if mode == "mean":
        a = (a / np.float32(len(Pm))).astype(np.float32)
    return a


def candidates(Pm, rows, watched=None, exclude_row=None, floor=None):
    """bool [n]: no member's watched flag, no exclude flag, no member rating below ``floor`` (a NaN rating is not below)"""
    ok = np.ones(Pm.shape[1], bool)
    if watched is not None:
        ok &= ~np.asarray(watched, bool)[rows].any(axis=0)
    if exclude_row is not None:
        ok &= ~np.asarray(exclude_row, bool)
    if floor is not None:
        with np.errstate(invalid="ignore"):
            ok &= ~(Pm < np.float32(floor)).any(axis=0)
    return ok


def rank(score, ok, k):
    """(idx int32 [k], score fp32 [k]): the candidates by score_key descending, ties in ascending index, -1 / NaN padded"""
    cand = np.nonzero(ok)[0]
    order = cand[np.lexsort((cand, -score_key(score[cand]).astype(np.int64)))][:k]
    idx = np.full(k, -1, np.int32)
    out = np.full(k, NAN, np.float32)
    idx[:len(order)] = order
    out[:len(order)] = score[order]
    return idx, out


def group_topk(P, offsets, member_row, k, mode="mean", floor=None, watched=None, exclude=None):
    """``P`` fp32 [n_users, n_anime]: the rating grid of the call's users; ``watched`` bool [n_users, n_anime],
    ``exclude`` bool [n_groups, n_anime].  Returns (idx int32 [n_groups, k], score fp32 [n_groups, k], member_p fp32
    [n_members, k]); an empty group's rows are padding."""
    P = np.asarray(P, np.float32)
    n_g = len(offsets) - 1
    idx = np.full((n_g, k), -1, np.int32)
    score = np.full((n_g, k), NAN, np.float32)
    member_p = np.full((len(member_row), k), NAN, np.float32)
    for g in range(n_g):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        if hi == lo:
            continue
        rows = np.asarray(member_row[lo:hi], np.int64)
        Pm = P[rows]
        ok = candidates(Pm, rows, watched, None if exclude is None else exclude[g], floor)
        idx[g], score[g] = rank(aggregate(Pm, mode), ok, k)
        have = idx[g] >= 0
        member_p[lo:hi][:, have] = Pm[:, idx[g][have]]
    return idx, score, member_p
