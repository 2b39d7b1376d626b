"""Restatement of the calibrated re-rank (include/anirec.h, anirec_calibrate_rerank and anirec_list_calibration): the
definition of the header comment, step for step, with no split of the sum.  A plain helper module, imported by the tests
the way ``mmr_restatement`` is.

    present  index >= 0 and a score that is not NaN
    state    q_c = picked candidates that carry category c, Q = sum q_c, P = sum p_c
    pen_i    for the list extended by candidate i (Q' = Q + pop_i, q' = q + b_i): 0 when P == 0, else 1 when Q' == 0,
             else float32(float64(num) / float64(den)), num = sum_c |p_c Q' - q'_c P|, den = 2 P Q' (integers)
    val_i    (omc * score_i) - (c * pen_i) in float32, omc = float32(1) - c, each product rounded, then the difference
    pick     the present, unpicked candidate with the largest val; ties (-0 == +0) to the lowest position; a NaN val
             after every number

``calibrate`` is one list with Python ints; ``rerank_lists`` is the same for every list of a call, the integers held in
int64 arrays (every value stays below 2**53) so that a 1024-candidate list takes seconds, not hours.
"""
import numpy as np

NAN32 = np.float32(np.nan)
PROFILE_MAX = 1 << 24


def miscalibration(p, q):
    """(num, den, pen) of a list whose category counts are ``q`` against the profile ``p`` (Python ints)."""
    p, q = [int(x) for x in p], [int(x) for x in q]
    P, Q = sum(p), sum(q)
    if P == 0:
        return 0, 1, np.float32(0.0)
    if Q == 0:
        return 1, 1, np.float32(1.0)
    num = sum(abs(pc * Q - qc * P) for pc, qc in zip(p, q))
    den = 2 * P * Q
    return num, den, np.float32(np.float64(num) / np.float64(den))


def unpack(cat_bits, n_cat):
    """bool [n_rows, n_cat] from uint32 [n_rows, ceil(n_cat/32)] bit words (bits at or above n_cat dropped)"""
    words = np.ascontiguousarray(cat_bits).view(np.uint32)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :n_cat].astype(bool)


def calibrate(cats, score, present, profile, k, c):
    """One list, Python ints.  ``cats`` [n][n_cat] bool: the category bits of the candidate at each position; ``score``
    [n] fp32; ``present`` [n] bool; ``profile`` [n_cat] ints.  Returns (pos int32 [k], score fp32 [k], pen fp32 [k]):
    -1 / NaN / NaN once no candidate is left.  Greedy: the first k' columns are the result for k' < k."""
    score = np.asarray(score, np.float32)
    c = np.float32(c)
    omc = np.float32(1.0) - c
    n = len(score)
    sets = [[j for j, bit in enumerate(row) if bit] for row in np.asarray(cats, bool)]
    p = [int(x) for x in profile]
    q = [0] * len(p)
    live = [bool(x) for x in present]
    out_pos = np.full(k, -1, np.int32)
    out_score = np.full(k, NAN32, np.float32)
    out_pen = np.full(k, NAN32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(k):
            best, best_val, best_pen = -1, None, None
            for i in range(n):
                if not live[i]:
                    continue
                q2 = list(q)
                for j in sets[i]:
                    q2[j] += 1
                pen = miscalibration(p, q2)[2]
                val = np.float32(omc * score[i]) - np.float32(c * pen)
                if best < 0 or (not np.isnan(val) and (np.isnan(best_val) or val > best_val)):
                    best, best_val, best_pen = i, val, pen
            if best < 0:
                break
            out_pos[s], out_score[s], out_pen[s] = best, score[best], best_pen
            live[best] = False
            for j in sets[best]:
                q[j] += 1
    return out_pos, out_score, out_pen


def _calibrate_int64(cats, score, present, profile, k, c):
    """``calibrate`` with the integers in int64 arrays: the same sums, term for term"""
    score = np.asarray(score, np.float32)
    c = np.float32(c)
    omc = np.float32(1.0) - c
    B = np.asarray(cats, bool).astype(np.int64)
    p = np.asarray(profile, np.int64)
    P = int(p.sum())
    q = np.zeros_like(p)
    Q = 0
    pop = B.sum(axis=1)
    BP = B * P
    live = np.asarray(present, bool).copy()
    out_pos = np.full(k, -1, np.int32)
    out_score = np.full(k, NAN32, np.float32)
    out_pen = np.full(k, NAN32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ls = omc * score
        for s in range(k):
            alive = np.flatnonzero(live)
            if len(alive) == 0:
                break
            Qp = Q + pop[alive]
            if P == 0:
                pen = np.zeros(len(alive), np.float32)
            else:
                T = np.multiply.outer(Qp, p)                    # p_c Q'
                T -= q * P                                      # - q_c P
                T -= BP[alive]                                  # - b_ic P
                np.abs(T, out=T)
                num, den = T.sum(axis=1), 2 * P * Qp
                pen = (num.astype(np.float64) / np.maximum(den, 1).astype(np.float64)).astype(np.float32)
                pen[Qp == 0] = np.float32(1.0)
            val = ls[alive] - c * pen
            numbers = ~np.isnan(val)
            at = int(np.flatnonzero(numbers & (val == val[numbers].max()))[0]) if numbers.any() else 0
            best = int(alive[at])
            out_pos[s], out_score[s], out_pen[s] = best, score[best], pen[at]
            live[best] = False
            q += B[best]
            Q += int(pop[best])
    return out_pos, out_score, out_pen


def bad_lists(n_rows, idx, profile):
    """bool [n_lists]: an index below -1 or at or above n_rows, or a profile entry that is negative or above 2**24"""
    idx, profile = np.asarray(idx, np.int64), np.asarray(profile, np.int64)
    return ((idx < -1) | (idx >= n_rows)).any(axis=1) | ((profile < 0) | (profile > PROFILE_MAX)).any(axis=1)


def rerank_lists(cat_bits, n_cat, cand_idx, cand_score, profile, k, c, one=_calibrate_int64):
    """The definition for every list of a call.  Returns (idx, pos, score, pen, err): each [n_lists, k], a bad list all
    -1 / -1 / NaN / NaN, err = 1 with a bad list."""
    cats = unpack(cat_bits, n_cat)
    cand_idx = np.asarray(cand_idx)
    cand_score = np.asarray(cand_score, np.float32)
    n_lists = len(cand_idx)
    idx = np.full((n_lists, k), -1, np.int32)
    pos = np.full((n_lists, k), -1, np.int32)
    score = np.full((n_lists, k), NAN32, np.float32)
    pen = np.full((n_lists, k), NAN32, np.float32)
    bad = bad_lists(len(cats), cand_idx, profile)
    for l in range(n_lists):
        if bad[l]:
            continue
        present = (cand_idx[l] >= 0) & ~np.isnan(cand_score[l])
        rows = cats[np.where(cand_idx[l] >= 0, cand_idx[l], 0)] & (cand_idx[l] >= 0)[:, None]
        pos[l], score[l], pen[l] = one(rows, cand_score[l], present, profile[l], k, c)
        idx[l] = np.where(pos[l] >= 0, cand_idx[l][np.maximum(pos[l], 0)], -1)
    return idx, pos, score, pen, int(bad.any())


def list_calibration(cat_bits, n_cat, lists, profile):
    """anirec_list_calibration: (num int64, den int64, pen fp32, err), each [n_lists]; -1 / -1 / NaN for a bad list"""
    cats = unpack(cat_bits, n_cat)
    lists = np.asarray(lists)
    n_lists = len(lists)
    num = np.full(n_lists, -1, np.int64)
    den = np.full(n_lists, -1, np.int64)
    pen = np.full(n_lists, NAN32, np.float32)
    bad = bad_lists(len(cats), lists, profile)
    for l in range(n_lists):
        if bad[l]:
            continue
        q = cats[lists[l][lists[l] >= 0]].sum(axis=0)
        num[l], den[l], pen[l] = miscalibration(profile[l], q)
    return num, den, pen, int(bad.any())
