"""NumPy restatement of the rank of a held-out anime (include/anirec.h, anirec_predict_rank) from a matrix of fp32
ratings, of the watched-bit table (anirec_seen_bits), and the search of a target in a whole ranking — the yardstick
the GPU tests hold ops.predict_rank to.  A plain helper module, imported the way ``metrics_restatement`` is."""
import numpy as np


def score_key(p):
    """The uint32 order key of fp32 ratings (score_key of the library): a larger rating has a larger key, -0.0 sorts
    just below +0.0, NaN (key 1) after every number."""
    p = np.asarray(p, np.float32)
    u = p.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key = np.maximum(key, np.uint32(2))
    return np.where(np.isnan(p), np.uint32(1), key).astype(np.uint32)


def pack(mask):
    """bool [..., n] -> uint32 bit words [..., ceil(n/32)] (bit a & 31 of word a >> 5)"""
    mask = np.asarray(mask, bool)
    pad = np.zeros(mask.shape[:-1] + ((-mask.shape[-1]) % 32,), bool)
    return np.packbits(np.concatenate([mask, pad], axis=-1), axis=-1, bitorder="little").view(np.uint32)


def unpack(bits, n):
    """uint32 bit words [..., w] -> bool [..., n]: bits past n are dropped"""
    b = np.ascontiguousarray(np.asarray(bits).view(np.uint32))
    return np.unpackbits(b.view(np.uint8), axis=-1, bitorder="little")[..., :n].astype(bool)


def seen_bits(user, anime, n_users, n_anime):
    bits = np.zeros((n_users, (n_anime + 31) // 32), np.uint32)
    user, anime = np.asarray(user, np.int64), np.asarray(anime, np.int64)
    np.bitwise_or.at(bits, (user, anime >> 5), np.uint32(1) << (anime & 31).astype(np.uint32))
    return bits


def ranks(P, target_row, target_anime, watched=None):
    """rank[t] = #{ j != a_t : not watched[row_t][j] and (key(P[row_t][j]) > key(p_t) or (== and j < a_t)) } and
    p[t] = P[row_t][a_t]; ``P``: fp32 [n_users, n_anime]; ``watched``: bool [n_users, n_anime] or None.  The
    target's own watched flag is ignored."""
    P = np.asarray(P, np.float32)
    n = P.shape[1]
    j = np.arange(n)
    out = np.zeros(len(target_row), np.int64)
    for t, (r, a) in enumerate(zip(target_row, target_anime)):
        key = score_key(P[r])
        ok = np.ones(n, bool) if watched is None else ~np.asarray(watched[r], bool)
        ok[a] = False
        out[t] = int((ok & ((key > key[a]) | ((key == key[a]) & (j < a)))).sum())
    return out, P[np.asarray(target_row), np.asarray(target_anime)]


def position(idx_row, a):
    """The position of anime ``a`` in one row of a whole ranking (-1 padded index list); it must be there once."""
    pos = np.nonzero(np.asarray(idx_row) == a)[0]
    assert len(pos) == 1, (a, idx_row)
    return int(pos[0])


def ranking_metrics(rank, ks):
    """Plain-Python float64 restatement of recs.ranking_metrics (one relevant anime per row: IDCG = 1)."""
    import math
    r = [int(x) for x in rank]
    n = len(r)
    mean = (lambda xs: sum(xs) / n) if n else (lambda xs: float("nan"))
    s = sorted(r)
    med = float("nan") if not n else (s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2]))
    return {"hit_rate": {k: mean([1.0 if x < k else 0.0 for x in r]) for k in ks},
            "ndcg": {k: mean([1.0 / math.log2(x + 2) if x < k else 0.0 for x in r]) for k in ks},
            "mrr": mean([1.0 / (x + 1) for x in r]), "mean_rank": mean([float(x) for x in r]),
            "median_rank": float(med), "n": n}
