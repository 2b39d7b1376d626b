"""NumPy restatement of the greedy MMR re-rank (include/anirec.h, anirec_mmr_rerank), in float32 on a GIVEN similarity
matrix: the definition of the header comment, step for step.  A plain helper module, imported by the tests the way
``foldin_restatement`` is.

    absent   index -1, NaN score, or a table row with a non-finite value       (``present_mask``)
    pen_i    0 while nothing is picked; sim(i, first) after the first pick; then sim(i, j) wherever it is larger
    val_i    (lam * score_i) - (oml * pen_i), oml = float32(1) - lam, each product rounded, then the difference
    pick     the present, unpicked candidate with the largest val; ties (-0 == +0) to the lowest position; a NaN val
             after every number
"""
import numpy as np

NAN32 = np.float32(np.nan)


def present_mask(What, cand_idx, cand_score):
    """bool [..., n_cand]: the candidates the definition calls present (``What``: the normalised table on the host)"""
    idx = np.asarray(cand_idx)
    row_ok = np.isfinite(np.asarray(What)).all(axis=1)
    return (idx >= 0) & ~np.isnan(np.asarray(cand_score)) & row_ok[np.where(idx >= 0, idx, 0)]


def mmr(S, score, present, k, lam):
    """One list.  ``S`` [n, n] fp32: S[i, j] = sim(i, j) of the candidates at positions i and j; ``score`` [n] fp32;
    ``present`` [n] bool.  Returns (pos int32 [k], score fp32 [k], pen fp32 [k]): -1 / NaN / NaN once no candidate is
    left.  Greedy: the first k' columns are the result for k' < k."""
    S = np.asarray(S, np.float32)
    score = np.asarray(score, np.float32)
    lam = np.float32(lam)
    oml = np.float32(1.0) - lam
    n = len(score)
    live = np.asarray(present, bool).copy()
    pen = np.zeros(n, np.float32)
    out_pos = np.full(k, -1, np.int32)
    out_score = np.full(k, NAN32, np.float32)
    out_pen = np.full(k, NAN32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ls = lam * score                                        # fp32 product, rounded
        for s in range(k):
            if not live.any():
                break
            val = ls - oml * pen                                # fp32 product rounded, then the fp32 difference
            numbers = live & ~np.isnan(val)
            if numbers.any():
                best = int(np.flatnonzero(numbers & (val == val[numbers].max()))[0])      # == : -0 ties with +0
            else:
                best = int(np.flatnonzero(live)[0])
            out_pos[s], out_score[s], out_pen[s] = best, score[best], pen[best]
            live[best] = False
            sim = S[:, best]
            pen = sim.copy() if s == 0 else np.where(sim > pen, sim, pen)
    return out_pos, out_score, out_pen


def rerank_lists(Sfull, What, cand_idx, cand_score, k, lam):
    """``mmr`` for every list of a call.  ``Sfull`` [n_rows, n_rows] fp32: the similarities of the table's rows
    (row q = ``ops.cosine_scores(What, q)``).  Returns (idx, pos, score, pen), each [n_lists, k]."""
    cand_idx = np.asarray(cand_idx)
    cand_score = np.asarray(cand_score, np.float32)
    pres = present_mask(What, cand_idx, cand_score)
    n_lists = len(cand_idx)
    idx = np.full((n_lists, k), -1, np.int32)
    pos = np.full((n_lists, k), -1, np.int32)
    score = np.full((n_lists, k), NAN32, np.float32)
    pen = np.full((n_lists, k), NAN32, np.float32)
    for l in range(n_lists):
        rows = np.where(cand_idx[l] >= 0, cand_idx[l], 0)
        pos[l], score[l], pen[l] = mmr(Sfull[np.ix_(rows, rows)], cand_score[l], pres[l], k, lam)
        idx[l] = np.where(pos[l] >= 0, cand_idx[l][np.maximum(pos[l], 0)], -1)
    return idx, pos, score, pen
