"""NumPy restatement of the explained lists (include/anirec.h, anirec_explain_lists), in float32 on a GIVEN similarity
matrix: the definition of the header comment, step for step.  A plain helper module, imported by the tests the way
``listeval_restatement`` is.

    contrib   weight[i] * sim(s, i): one np.float32 product
    order     a stable sort on -contrib with the NaNs removed: contrib descending, ties (-0 == +0) to the lowest
              history position, +-inf ordinary numbers, a NaN contrib never picked
    rank r    pos = the entry's position in the history, sim, contrib; -1 / NaN / NaN (0x7FC00000) past the pickable
              entries and for an absent slot
"""
import numpy as np

NAN32 = np.float32(np.nan)


def explain(S_rows, weight, present, m):
    """One list.  ``S_rows`` [k, n] fp32: S_rows[s, i] = sim(slot s, history entry i); ``weight`` [n] fp32; ``present``
    [k] bool.  Returns (pos int32 [k, m], sim fp32 [k, m], contrib fp32 [k, m])."""
    present = np.asarray(present, bool)
    k, m = len(present), int(m)
    weight = np.asarray(weight, np.float32).reshape(-1)
    S_rows = np.asarray(S_rows, np.float32).reshape(k, len(weight))
    pos = np.full((k, m), -1, np.int32)
    sim = np.full((k, m), NAN32, np.float32)
    contrib = np.full((k, m), NAN32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(k):
            if not present[s]:
                continue
            c = np.multiply(weight, S_rows[s], dtype=np.float32)
            live = np.flatnonzero(~np.isnan(c))
            pick = live[np.argsort(-c[live], kind="stable")][:m]
            pos[s, :len(pick)] = pick
            sim[s, :len(pick)] = S_rows[s, pick]
            contrib[s, :len(pick)] = c[pick]
    return pos, sim, contrib


def explain_lists(Sfull, list_idx, offsets, hist_idx, weight, m):
    """``explain`` for every list of a call.  ``Sfull`` [n_rows, n_rows] fp32: the similarities of the table's rows (row
    q = ``ops.cosine_scores(What, q)``); list l's history is entries offsets[l] .. offsets[l + 1] - 1 of (hist_idx,
    weight).  Returns (pos, sim, contrib), each [n_lists, k, m]."""
    list_idx = np.asarray(list_idx)
    offsets = np.asarray(offsets, np.int64)
    hist_idx = np.asarray(hist_idx, np.int64)
    weight = np.asarray(weight, np.float32)
    n_lists, k = list_idx.shape
    pos = np.full((n_lists, k, m), -1, np.int32)
    sim = np.full((n_lists, k, m), NAN32, np.float32)
    contrib = np.full((n_lists, k, m), NAN32, np.float32)
    for l in range(n_lists):
        h = hist_idx[offsets[l]:offsets[l + 1]]
        rows = np.where(list_idx[l] >= 0, list_idx[l], 0)
        pos[l], sim[l], contrib[l] = explain(Sfull[np.ix_(rows, h)], weight[offsets[l]:offsets[l + 1]], list_idx[l] >= 0, m)
    return pos, sim, contrib
