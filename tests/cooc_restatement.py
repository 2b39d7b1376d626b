"""NumPy restatement of the item-kNN calls (include/anirec.h: anirec_cooc_scores, anirec_rows_topk, anirec_rows_rank,
anirec_itemknn_scores): the definitions of the header comment, step for step.  A plain helper module, imported by the
tests the way ``kmeans_restatement`` is; the ``ops_*`` functions at the end have the signatures of the ``ops`` wrappers
on NumPy arrays, for the CPU tests that run the host logic without a device.

    bits     uint32 [n_items, ceil(n_users/32)]; bit u & 31 of word u >> 5; bits at positions >= n_users ignored
    pop, c   popcounts over the valid bits
    den      np.float64 operations one at a time (NumPy never fuses): sqrt(pop_q * pop_j) + shrink;
             float64(int64(pop_q + pop_j - c)) + shrink;  float64(pop_q) + shrink
    sim      float32(float64(c) / den) where c >= max(1, min_support), else +0
    key      NaN -> 1; else the fp32 bits u: sign set -> ~u, clear -> u | 0x80000000; max(., 2); larger first, then
             ascending index (a stable sort)
    term     np.rint(float64(w) * float64(sim) * 2**30) as int64;  out = float32(float64(S) * 2**-30)
"""
import numpy as np

COSINE, JACCARD, CONFIDENCE = 0, 1, 2
MEASURES = {"cosine": COSINE, "jaccard": JACCARD, "confidence": CONFIDENCE}
NAN32 = np.uint32(0x7FC00000).view(np.float32)
Q_SCALE = float(2 ** 30)
MAX_TERM = 1024.0


def pack_bits(M):
    """bool [n_rows, n_cols] -> uint32 [n_rows, ceil(n_cols/32)], bit c & 31 of word c >> 5."""
    M = np.asarray(M, bool)
    n, m = M.shape
    w = (m + 31) // 32
    P = np.zeros((n, w * 32), bool)
    P[:, :m] = M
    return (P.reshape(n, w, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_bits(bits, n_cols):
    """The inverse: bool [n_rows, n_cols]; whatever lies at positions >= n_cols is dropped."""
    b = np.ascontiguousarray(bits).view(np.uint32)
    M = ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool)
    return M.reshape(b.shape[0], -1)[:, :n_cols]


def cooc_scores(bits, n_users, queries, measure=COSINE, shrink=0.0, min_support=1):
    """Returns (sim fp32 [nq, n], count int32 [nq, n], excl uint32 [nq, ceil(n/32)], pop int32 [n], err)."""
    L = unpack_bits(bits, n_users).astype(np.float64)         # 0 / 1: sums below 2**53 are exact in float64 (and fast)
    n = L.shape[0]
    pop = L.sum(axis=1).astype(np.int64)
    q = np.asarray(queries, np.int64).reshape(-1)
    ok_q = (q >= 0) & (q < n)
    qs = np.where(ok_q, q, 0)
    c = (L[qs] @ L.T).astype(np.int64)
    pq = pop[qs][:, None].astype(np.float64)
    pj = pop[None, :].astype(np.float64)
    shrink = np.float64(shrink)
    if measure == COSINE:
        den = np.sqrt(pq * pj) + shrink
    elif measure == JACCARD:
        den = (pop[qs][:, None] + pop[None, :] - c).astype(np.float64) + shrink
    else:
        assert measure == CONFIDENCE
        den = (pq + np.zeros_like(pj)) + shrink
    sup = c >= max(1, int(min_support))
    with np.errstate(divide="ignore", invalid="ignore"):
        sim = np.where(sup, (c.astype(np.float64) / den).astype(np.float32), np.float32(0.0)).astype(np.float32)
    excl = ~sup | (np.arange(n)[None, :] == q[:, None])
    cnt = c.astype(np.int32)
    sim[~ok_q] = NAN32
    cnt[~ok_q] = -1
    excl[~ok_q] = True
    return sim, cnt, pack_bits(excl), pop.astype(np.int32), int((~ok_q).any())


def score_key(s):
    """The select's key of fp32 scores, uint32."""
    s = np.ascontiguousarray(s, np.float32)
    u = s.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    k = np.maximum(k, np.uint32(2))
    return np.where(np.isnan(s), np.uint32(1), k).astype(np.uint32)


def rows_topk(scores, k, n=None, self_idx=None, keep=None, wbits=None):
    """Returns (idx int32 [nq, k], score fp32 [nq, k]) padded with -1 / NaN."""
    S = np.asarray(scores, np.float32)
    nq, ld = S.shape
    n = ld if n is None else int(n)
    idx = np.full((nq, k), -1, np.int32)
    out = np.full((nq, k), NAN32, np.float32)
    W = None if wbits is None else unpack_bits(np.asarray(wbits), n)
    for t in range(nq):
        cand = np.ones(n, bool)
        if self_idx is not None and 0 <= int(self_idx[t]) < n:
            cand[int(self_idx[t])] = False
        if keep is not None:
            cand &= np.asarray(keep).reshape(-1)[:n] != 0
        if W is not None:
            cand &= ~W[t]
        j = np.flatnonzero(cand)
        order = j[np.argsort(-score_key(S[t, j]).astype(np.int64), kind="stable")][:k]
        idx[t, :len(order)] = order
        out[t, :len(order)] = S[t, order]
    return idx, out


def rows_rank(scores, ld, n_anime, watched, n_users, target_row, target_anime):
    """``scores``: a flat fp32 array; row r starts at r * ld (ld == 0: one shared vector).  Returns (rank int32, err)."""
    sc = np.asarray(scores, np.float32).reshape(-1)
    W = None if watched is None else unpack_bits(np.asarray(watched), n_anime)
    tr, ta = np.asarray(target_row, np.int64), np.asarray(target_anime, np.int64)
    rank = np.full(len(tr), -1, np.int32)
    err = 0
    j = np.arange(n_anime)
    for t in range(len(tr)):
        r, a = int(tr[t]), int(ta[t])
        if not (0 <= r < n_users and 0 <= a < n_anime):
            err = 1
            continue
        key = score_key(sc[r * ld:r * ld + n_anime])
        before = (key > key[a]) | ((key == key[a]) & (j < a))
        seen = W[r] if W is not None else np.zeros(n_anime, bool)
        rank[t] = int((before & ~seen & (j != a)).sum())
    return rank, err


def itemknn_scores(nbr_idx, nbr_sim, offsets, hist_idx, hist_w=None):
    """Returns (out fp32 [n_lists, n_items], err)."""
    ni, ns = np.asarray(nbr_idx, np.int64), np.asarray(nbr_sim, np.float32)
    n, K = ni.shape
    off = np.asarray(offsets, np.int64).reshape(-1)
    hi = np.asarray(hist_idx, np.int64).reshape(-1)
    hw = None if hist_w is None else np.asarray(hist_w, np.float32).reshape(-1)
    n_l = len(off) - 1
    out = np.zeros((n_l, n), np.float32)
    err = 0
    for l in range(n_l):
        lo, hi_ = int(off[l]), int(off[l + 1])
        if lo < 0 or hi_ < lo or hi_ > len(hi):
            err = 1
            out[l] = NAN32
            continue
        S = np.zeros(n, np.int64)
        for e in range(lo, hi_):
            i = int(hi[e])
            if not 0 <= i < n:
                err = 1
                continue
            w = np.float64(1.0 if hw is None else hw[e])
            for s in range(K):
                j = int(ni[i, s])
                if j < 0:
                    continue
                if j >= n:
                    err = 1
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    prod = w * np.float64(ns[i, s])
                if not abs(prod) <= MAX_TERM:
                    err = 1
                    continue
                S[j] += np.int64(np.rint(prod * Q_SCALE))
        out[l] = (S.astype(np.float64) * (1.0 / Q_SCALE)).astype(np.float32)
    return out, err


# ---- the wrappers' signatures on NumPy arrays (tests that run host logic with ``ops`` replaced) ----------------------
def ops_seen_bits(user_idx, anime_idx, n_users, n_anime, device=None):
    u, a = np.asarray(user_idx, np.int64).reshape(-1), np.asarray(anime_idx, np.int64).reshape(-1)
    if u.size and (u.min() < 0 or u.max() >= n_users or a.min() < 0 or a.max() >= n_anime):
        raise ValueError("seen_bits: user or anime index out of range")
    M = np.zeros((int(n_users), int(n_anime)), bool)
    M[u, a] = True
    return pack_bits(M).view(np.int32)


def ops_cooc_scores(bits, n_users, queries, measure="cosine", shrink=0.0, min_support=1, count=False, excl=False,
                    pop=False):
    sim, cnt, ex, pp, err = cooc_scores(bits, n_users, queries, MEASURES[str(measure).lower()], shrink, min_support)
    if err:
        raise ValueError("cooc_scores: query item out of range")
    return sim, cnt if count else None, ex.view(np.int32) if excl else None, pp if pop else None


def ops_rows_topk(scores, k, n=None, self_idx=None, keep=None, wbits=None):
    return rows_topk(scores, int(k), n, self_idx, keep, wbits)


def ops_rows_rank(scores, target_row, target_anime, watched_bits=None):
    S = np.asarray(scores, np.float32)
    rank, err = rows_rank(S, S.shape[1], S.shape[1], watched_bits, S.shape[0], target_row, target_anime)
    if err:
        raise ValueError("rows_rank: target_row or target_anime out of range")
    return rank


def ops_itemknn_scores(nbr_idx, nbr_sim, offsets, hist_idx, hist_w=None):
    out, err = itemknn_scores(nbr_idx, nbr_sim, offsets, hist_idx, hist_w)
    if err:
        raise ValueError("itemknn_scores: out of range")
    return out
