"""NumPy restatement of the RP3beta graph baseline (include/anirec.h: anirec_wcooc_scores; recs.rp3_*), the
definitions step for step.  A plain helper module, imported by the tests the way ``cooc_restatement`` is.

    bits     uint32 [n_items, ceil(n_users/32)]; bit u & 31 of word u >> 5; bits at positions >= n_users ignored
    q_u      0 where deg(u) = 0, else max(1, rint(16383 * (d_min / deg(u)) ** alpha)) in fp64, d_min the smallest
             positive degree
    S        int64: the sum of q_u over the users set in both rows (a weight outside 0 .. 16383 counts as 0: flag)
    w        float32((float64(S) * row_scale[q]) * col_scale[j]), np.float64 operations one at a time; +0 where S = 0
    excl     S == 0 or j == q; a query outside the items: a NaN row, sums of -1, every bit j < n_items, flag
    scales   pop ** -alpha (rows) and pop ** -beta (columns) in fp64, 0 where pop = 0
    top-K    larger first, ties by index, never the item itself nor an item with S = 0 (cooc_restatement.rows_topk)
    scale    all kept weights times the power of two that puts the largest of them in [256, 512)
    scores   cooc_restatement.itemknn_scores over the tables / ease_restatement.ease_scores over the dense W
"""
import numpy as np

import cooc_restatement as C
import ease_restatement as E

MAX_Q = 16383
NAN32 = C.NAN32


def user_weights(deg, alpha):
    deg = np.asarray(deg, np.int64).reshape(-1)
    q = np.zeros(len(deg), np.int32)
    pos = deg > 0
    if pos.any():
        d_min = np.float64(deg[pos].min())
        q[pos] = np.maximum(1.0, np.rint(16383.0 * (d_min / deg[pos].astype(np.float64)) ** np.float64(alpha))).astype(np.int32)
    return q


def pop_scales(pop, alpha, beta):
    """(row_scale, col_scale) fp64 [n_items]"""
    p = np.asarray(pop, np.int64).astype(np.float64)
    ok = p > 0
    row, col = np.zeros(len(p)), np.zeros(len(p))
    row[ok] = p[ok] ** np.float64(-float(alpha))
    col[ok] = p[ok] ** np.float64(-float(beta))
    return row, col


def wcooc_scores(bits, n_users, user_q, queries, row_scale=None, col_scale=None):
    """Returns (w fp32 [nq, n], sum int64 [nq, n], excl uint32 [nq, ceil(n/32)], err)."""
    L = C.unpack_bits(bits, n_users).astype(np.float64)      # 0 / 1; the sums stay below 2**53: exact in float64
    n = L.shape[0]
    uq = np.asarray(user_q, np.int64).reshape(-1)
    assert uq.shape == (n_users,)
    bad_w = (uq < 0) | (uq > MAX_Q)
    uq = np.where(bad_w, 0, uq)
    q = np.asarray(queries, np.int64).reshape(-1)
    ok_q = (q >= 0) & (q < n)
    qs = np.where(ok_q, q, 0)
    S = ((L[qs] * uq.astype(np.float64)[None, :]) @ L.T).astype(np.int64)
    rs = np.ones(n) if row_scale is None else np.asarray(row_scale, np.float64)
    cs = np.ones(n) if col_scale is None else np.asarray(col_scale, np.float64)
    with np.errstate(all="ignore"):
        a = S.astype(np.float64) * rs[qs][:, None]
        w = (a * cs[None, :]).astype(np.float32)
    w = np.where(S != 0, w, np.float32(0.0)).astype(np.float32)
    excl = (S == 0) | (np.arange(n)[None, :] == q[:, None])
    w[~ok_q] = NAN32
    S[~ok_q] = -1
    excl[~ok_q] = True
    return w, S, C.pack_bits(excl), int((~ok_q).any() or bad_w.any())


def literal_wcooc(B, user_q, queries, row_scale, col_scale):
    """The same by literal loops over a bool matrix (valid queries and weights only): (w, S, excl bool)."""
    B = np.asarray(B, bool)
    n, m = B.shape
    nq = len(queries)
    S = np.zeros((nq, n), np.int64)
    w = np.zeros((nq, n), np.float32)
    ex = np.zeros((nq, n), bool)
    for t, i in enumerate(queries):
        for j in range(n):
            s = 0
            for u in range(m):
                if B[i, u] and B[j, u]:
                    s += int(user_q[u])
            S[t, j] = s
            if s:
                w[t, j] = np.float32(np.float64(np.float64(s) * np.float64(row_scale[i])) * np.float64(col_scale[j]))
            ex[t, j] = s == 0 or j == i
    return w, S, ex


def pow2_scale(values):
    """The fp32 power of two that puts the largest finite positive value in [256, 512); 1 when there is none."""
    v = np.asarray(values, np.float32).reshape(-1)
    v = v[np.isfinite(v)]
    m = float(v.max()) if v.size else 0.0
    if not m > 0.0:
        return np.float32(1.0)
    _, ex = np.frexp(m)                 # m = f * 2**ex, f in [0.5, 1): m in [2**(ex - 1), 2**ex)
    return np.float32(np.ldexp(1.0, 9 - int(ex)))


def rp3_fit(B, alpha=1.0, beta=0.3, neighbours=100, quantised=True):
    """The model of a bool liked matrix [n_items, n_users]: {"nbr_idx", "nbr_sim"} (neighbours > 0) or {"W"}
    (neighbours = 0), plus pop, deg, user_q, scale.  ``quantised=False``: the unquantised fp64 weights deg ** -alpha in
    place of q_u (what the quantisation is measured against; no kernel computes it)."""
    B = np.asarray(B, bool)
    n, m = B.shape
    pop, deg = B.sum(1).astype(np.int64), B.sum(0).astype(np.int64)
    row, col = pop_scales(pop, alpha, beta)
    uq = user_weights(deg, alpha)
    if quantised:
        w, S, ex, err = wcooc_scores(C.pack_bits(B), m, uq, np.arange(n), row, col)
        assert not err
    else:
        L = B.astype(np.float64)
        uw = np.where(deg > 0, np.maximum(deg, 1).astype(np.float64) ** -float(alpha), 0.0)
        Sf = (L * uw[None, :]) @ L.T
        w = ((Sf * row[:, None]) * col[None, :]).astype(np.float32)
        ex = C.pack_bits((Sf == 0) | np.eye(n, dtype=bool))
    fit = dict(pop=pop, deg=deg, user_q=uq, alpha=alpha, beta=beta, neighbours=neighbours)
    if neighbours:
        idx, sim = C.rows_topk(w, neighbours, wbits=ex)
        sc = pow2_scale(sim[idx >= 0])
        fit.update(nbr_idx=idx, nbr_sim=(sim * sc).astype(np.float32), scale=sc)
    else:
        W = w.copy()
        W[np.diag_indices(n)] = np.float32(0.0)
        sc = pow2_scale(W)
        fit.update(W=(W * sc).astype(np.float32), scale=sc)
    return fit


def rp3_scores(fit, offsets, hist_idx, hist_w=None):
    """(score rows fp32 [n_lists, n_items], err) through the existing fixed-point sums"""
    if "W" in fit:
        return E.ease_scores(fit["W"], offsets, hist_idx, hist_w)
    return C.itemknn_scores(fit["nbr_idx"], fit["nbr_sim"], offsets, hist_idx, hist_w)


def rp3_similar(fit, queries, k):
    """(idx, score): the k largest weights of each query's row, never the query itself"""
    q = np.asarray(queries, np.int64).reshape(-1)
    if "W" in fit:
        return C.rows_topk(fit["W"][q], k, self_idx=q)
    n = len(fit["nbr_idx"])
    rows = np.zeros((len(q), n), np.float32)
    cand = np.zeros((len(q), n), bool)
    for t, i in enumerate(q):
        j = fit["nbr_idx"][i]
        rows[t, j[j >= 0]] = fit["nbr_sim"][i][j >= 0]
        cand[t, j[j >= 0]] = True
    return C.rows_topk(rows, k, wbits=C.pack_bits(~cand))
