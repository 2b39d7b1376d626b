"""The exact t-SNE of include/anirec.h ("MAPPED TABLES") restated in NumPy and Python ints, and a plain fp64 t-SNE
(analytic gradient, float sums) as the yardstick of its accuracy.  A plain helper module, imported by the tests.

``forces`` / ``fit`` follow the header term by term: the fp32 pair chain with every operation rounded on its own (NumPy
never contracts), I(p) = rint(p * 2^30) as int64, row sums as int64, Z as a Python int (the two-word sum of the
library, whatever its size), and the update as single fp64 operations.  Nothing here knows about tiles, lanes or splits.
"""
import numpy as np

S = np.float32(2.0 ** 30)
MAX_COORD = np.float32(2.0 ** 60)
F32, F64 = np.float32, np.float64
TWO64 = 2.0 ** 64


def csr_from_dense(P):
    """(offsets int64, idx int32, val fp32) of the non-zero entries of a dense [n, n] array, rows in column order"""
    P = np.asarray(P)
    n = P.shape[0]
    offsets = np.zeros(n + 1, np.int64)
    idx, val = [], []
    for i in range(n):
        js = np.flatnonzero(P[i])
        idx.append(js)
        val.append(P[i, js])
        offsets[i + 1] = offsets[i] + len(js)
    return offsets, np.concatenate(idx).astype(np.int32) if n else np.zeros(0, np.int32), \
        np.concatenate(val).astype(np.float32)


def usable(Y):
    with np.errstate(invalid="ignore"):
        return (np.abs(Y) <= MAX_COORD).all(axis=1)


def _I(p):
    """rint(p * 2^30) as int64: the product is exact in fp32"""
    return np.rint(p * S).astype(np.int64)


def forces(Y, offsets, idx, val, chunk=512):
    """The integer sums at Y: (Rx, Ry, Ax, Ay int64 [n], Z Python int, info int)."""
    Y = np.ascontiguousarray(Y, F32)
    n = len(Y)
    ok = usable(Y)
    info = 0 if ok.all() else 1
    Ys = np.where(ok[:, None], Y, F32(0))
    Rx, Ry = np.zeros(n, np.int64), np.zeros(n, np.int64)
    Z = 0
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for b in range(0, n, chunk):
            e = min(n, b + chunk)
            dx = Ys[b:e, None, 0] - Ys[None, :, 0]
            dy = Ys[b:e, None, 1] - Ys[None, :, 1]
            d2 = dx * dx + dy * dy          # two rounded products, one rounded sum
            q = F32(1) / (F32(1) + d2)
            w = q * q
            pair = ok[b:e, None] & ok[None, :]
            pair[np.arange(e - b), np.arange(b, e)] = False     # excluded by index
            Z += int(np.where(pair, _I(q), 0).sum(dtype=np.int64))  # (a chunk stays far inside int64)
            Rx[b:e] = np.where(pair, _I(w * dx), 0).sum(axis=1)
            Ry[b:e] = np.where(pair, _I(w * dy), 0).sum(axis=1)
    Ax, Ay = np.zeros(n, np.int64), np.zeros(n, np.int64)
    offsets = np.asarray(offsets, np.int64)
    idx = np.asarray(idx, np.int64)
    val = np.asarray(val, F32)
    nnz = len(idx)
    b, e = offsets[:-1], offsets[1:]
    bad_row = (b < 0) | (e > nnz) | (b > e)
    if bad_row.any():
        info |= 4
    cnt = np.where(bad_row | ~ok, 0, e - b)
    i = np.repeat(np.arange(n), cnt)                                        # the row of every entry that counts
    t = np.repeat(np.where(cnt > 0, b, 0) - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
    j, v = idx[t], val[t]
    bad_j = (j < 0) | (j >= n) | (j == i)
    with np.errstate(invalid="ignore"):
        bad_v = ~bad_j & ~((v >= 0) & (v <= 2))
    if bad_j.any():
        info |= 4
    if bad_v.any():
        info |= 2
    keep = ~bad_j & ~bad_v
    keep[keep] &= ok[j[keep]]
    i, j, v = i[keep], j[keep], v[keep]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        dx = Y[i, 0] - Y[j, 0]
        dy = Y[i, 1] - Y[j, 1]
        d2 = dx * dx + dy * dy
        q = F32(1) / (F32(1) + d2)
        a = v * q
        np.add.at(Ax, i, _I(a * dx))
        np.add.at(Ay, i, _I(a * dy))
    return Rx, Ry, Ax, Ay, Z, info


def z_words(Z):
    return np.array([Z & (2 ** 64 - 1), Z >> 64], np.uint64)


def update(Y, V, G, Rx, Ry, Ax, Ay, Z, e, mom, lr):
    """One update of every row: (Y fp32, V fp64, G fp64), each operation one rounded fp64 operation."""
    n = len(Y)
    zd = F64(float(Z >> 64)) * F64(TWO64) + F64(float(Z & (2 ** 64 - 1)))   # float(int) rounds to nearest even
    den_a = F64(2147483648.0) * F64(n)
    A = np.stack([Ax, Ay], axis=1).astype(F64)
    R = np.stack([Rx, Ry], axis=1).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        att = (F64(e) * A) / den_a
        rep = R / zd if zd > 0 else np.zeros_like(R)
        grad = F64(4.0) * (att - rep)
        inc = np.sign(grad) != np.sign(V)
        G = np.where(inc, G + F64(0.2), G * F64(0.8))
        G = np.where(G < 0.01, F64(0.01), G)
        V = F64(mom) * V - (F64(lr) * G) * grad
        Y = (Y.astype(F64) + V).astype(F32)
    return Y, V, G


def fit(Y0, offsets, idx, val, iters, exag_iters=250, exaggeration=12.0, lr=50.0, snapshots=()):
    """``iters`` iterations from Y0: (Y, V, G, info), or with ``snapshots`` a dict {iterations done: (Y, V, G, info)}."""
    Y = np.ascontiguousarray(Y0, F32).copy()
    V, G = np.zeros((len(Y), 2), F64), np.ones((len(Y), 2), F64)
    info, out = 0, {}
    for t in range(iters):
        Rx, Ry, Ax, Ay, Z, bits = forces(Y, offsets, idx, val)
        info |= bits
        early = t < exag_iters
        Y, V, G = update(Y, V, G, Rx, Ry, Ax, Ay, Z, exaggeration if early else 1.0, 0.5 if early else 0.8, lr)
        if t + 1 in snapshots:
            out[t + 1] = (Y.copy(), V.copy(), G.copy(), info)
    return out if snapshots else (Y, V, G, info)


# ---- the affinities (the NumPy twin of recs.map_affinities' bisection and symmetrisation) ------------------------------
BISECT_STEPS = 64


def conditional_p(d2, perplexity, steps=BISECT_STEPS):
    """p(j|i) over each row's neighbour distances d2 [n, k] fp64: beta by ``steps`` bisection steps on the entropy,
    bracket [0, inf) doubled while open — the arithmetic of recs._map_bandwidths, in NumPy.  Returns (p [n, k], beta)."""
    d2 = np.asarray(d2, F64)
    n = len(d2)
    target = np.log(F64(perplexity))
    d0 = d2 - d2.min(axis=1, keepdims=True)
    beta = np.ones(n, F64)
    lo = np.zeros(n, F64)
    hi = np.full(n, np.inf, F64)
    for _ in range(steps):
        p = np.exp(-d0 * beta[:, None])
        s = p.sum(axis=1)
        h = np.log(s) + beta * (d0 * p).sum(axis=1) / s
        high = h > target                       # too flat: beta must grow
        lo = np.where(high, beta, lo)
        hi = np.where(high, hi, beta)
        beta = np.where(np.isinf(hi), beta * 2.0, (lo + hi) / 2.0)
    p = np.exp(-d0 * beta[:, None])
    return p / p.sum(axis=1, keepdims=True), beta


def row_perplexity(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp(-np.where(p > 0, p * np.log(p), 0.0).sum(axis=1))


def symmetrise(nbr, p):
    """P' = p(j|i) + p(i|j) as CSR (offsets int64, idx int32 ascending in a row, val fp32) from neighbour lists
    nbr [n, k] (-1 = none) and p [n, k] fp64."""
    n = len(nbr)
    rows = np.repeat(np.arange(n), nbr.shape[1])
    cols = nbr.reshape(-1).astype(np.int64)
    vals = np.asarray(p, F64).reshape(-1)
    keep = cols >= 0
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    key = np.concatenate([rows * n + cols, cols * n + rows])
    v2 = np.concatenate([vals, vals])
    order = np.argsort(key, kind="stable")
    key, v2 = key[order], v2[order]
    uniq, first = np.unique(key, return_index=True)
    summed = np.add.reduceat(v2, first) if len(key) else np.zeros(0)
    offsets = np.zeros(n + 1, np.int64)
    np.add.at(offsets, uniq // n + 1, 1)
    return np.cumsum(offsets), (uniq % n).astype(np.int32), summed.astype(np.float32)


def dense_affinities(X, perplexity):
    """The affinities of unit rows X with every other row as neighbour (the planted cases): CSR of P'."""
    X = np.asarray(X, F64)
    n = len(X)
    d2 = 2.0 - 2.0 * (X @ X.T)
    nbr = np.array([np.delete(np.arange(n), i) for i in range(n)])
    p, _ = conditional_p(np.take_along_axis(d2, nbr, axis=1), perplexity)
    return symmetrise(nbr, p)


# ---- the fp64 yardstick ----------------------------------------------------------------------------------------------
def dense_P(offsets, idx, val, n):
    """P = P' / (2 n) as a dense fp64 matrix"""
    P = np.zeros((n, n), F64)
    for i in range(n):
        P[i, idx[offsets[i]:offsets[i + 1]]] = val[offsets[i]:offsets[i + 1]]
    return P / (2.0 * n)


def kl_fp64(Y, P):
    Y = np.asarray(Y, F64)
    d2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    q = 1.0 / (1.0 + d2)
    np.fill_diagonal(q, 0.0)
    Q = q / q.sum()
    m = P > 0
    return float((P[m] * np.log(P[m] / Q[m])).sum())


def sums_fp64(Y, P):
    """(R [n, 2] = sum_j q^2 (yi - yj), A [n, 2] = sum_j P q (yi - yj), Z = sum q) in fp64 from float sums"""
    Y = np.asarray(Y, F64)
    d = Y[:, None, :] - Y[None, :, :]
    q = 1.0 / (1.0 + (d ** 2).sum(-1))
    np.fill_diagonal(q, 0.0)
    return ((q * q)[:, :, None] * d).sum(1), ((P * q)[:, :, None] * d).sum(1), q.sum()


def grad_fp64(Y, P, exaggeration=1.0):
    R, A, Z = sums_fp64(Y, P)
    return 4.0 * (exaggeration * A - R / Z)


def fit_fp64(Y0, P, iters, exag_iters=250, exaggeration=12.0, lr=50.0):
    """The same dynamics in plain fp64 with float sums (the yardstick of the final KL)"""
    Y = np.asarray(Y0, F64).copy()
    V, G = np.zeros_like(Y), np.ones_like(Y)
    for t in range(iters):
        early = t < exag_iters
        grad = grad_fp64(Y, P, exaggeration if early else 1.0)
        inc = np.sign(grad) != np.sign(V)
        G = np.maximum(np.where(inc, G + 0.2, G * 0.8), 0.01)
        V = (0.5 if early else 0.8) * V - lr * G * grad
        Y = Y + V
    return Y


# ---- the planted cases ------------------------------------------------------------------------------------------------
PLANTED = ((5, 30, 32, 10.0), (8, 40, 32, 15.0), (5, 30, 128, 10.0))   # clusters, rows each, D, perplexity


def planted(clusters, per, D, seed=0):
    """unit rows around random unit centres with 0.045 N(0, I) noise, renormalised: (X fp32 [n, D], label [n])"""
    rng = np.random.default_rng(1000 + seed)
    C = rng.standard_normal((clusters, D))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    label = np.repeat(np.arange(clusters), per)
    X = C[label] + 0.045 * rng.standard_normal((clusters * per, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X.astype(np.float32), label


def y0(n, seed=0):
    return (1e-4 * np.random.default_rng(seed).standard_normal((n, 2))).astype(np.float32)


def auto_lr(n, exaggeration=12.0):
    return max(n / exaggeration / 4.0, 50.0)


def knn_purity(Y, label, k=5):
    Y = np.asarray(Y, F64)
    d2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    nn = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return float((label[nn] == label[:, None]).mean())
