"""NumPy restatement of the list similarity structure (include/anirec.h, anirec_list_similarity), in float32 on a GIVEN
similarity matrix: the definition of the header comment, step for step.  A plain helper module, imported by the tests the
way ``mmr_restatement`` is.

    present   a slot whose index is not -1; a repeated index is two slots
    sim_sum   ((0 + sim(s, j1)) + sim(s, j2)) + ... over the present slots j1 < j2 < ... before s, fp32 adds in that order
    sim_max   sim(s, j1), then sim(s, j) wherever it is larger (a NaN replaces nothing): mmr's pen rule
    both 0 with no present slot before s; both NaN (0x7FC00000) for an absent slot
"""
import numpy as np

NAN32 = np.float32(np.nan)


def similarity(S, present):
    """One list.  ``S`` [k, k] fp32: S[s, j] = sim(s, j) of the slots at positions s and j; ``present`` [k] bool.
    Returns (sim_max fp32 [k], sim_sum fp32 [k])."""
    S = np.asarray(S, np.float32)
    present = np.asarray(present, bool)
    k = len(present)
    sim_max = np.full(k, NAN32, np.float32)
    sim_sum = np.full(k, NAN32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(k):
            if not present[s]:
                continue
            x = S[s, np.flatnonzero(present[:s])]               # sim(s, j) of the present slots before s, ascending j
            if len(x) == 0:
                sim_max[s] = sim_sum[s] = 0
                continue
            # np.add.accumulate in float32 IS the sequential sum: out[i] = out[i - 1] + x[i], each add rounded
            sim_sum[s] = np.add.accumulate(np.concatenate([np.zeros(1, np.float32), x]), dtype=np.float32)[-1]
            # "replaced when sim > current": a NaN first stays; otherwise the FIRST of the values equal to the largest
            # number (== : a later +0 does not replace a -0, a NaN never compares)
            sim_max[s] = x[0] if np.isnan(x[0]) else x[np.flatnonzero(x == np.nanmax(x))[0]]
    return sim_max, sim_sum


def similarity_lists(Sfull, list_idx):
    """``similarity`` for every list of a call.  ``Sfull`` [n_rows, n_rows] fp32: the similarities of the table's rows
    (row q = ``ops.cosine_scores(What, q)``).  Returns (sim_max, sim_sum), each [n_lists, k]."""
    list_idx = np.asarray(list_idx)
    n_lists, k = list_idx.shape
    sim_max = np.full((n_lists, k), NAN32, np.float32)
    sim_sum = np.full((n_lists, k), NAN32, np.float32)
    for l in range(n_lists):
        rows = np.where(list_idx[l] >= 0, list_idx[l], 0)
        sim_max[l], sim_sum[l] = similarity(Sfull[np.ix_(rows, rows)], list_idx[l] >= 0)
    return sim_max, sim_sum
