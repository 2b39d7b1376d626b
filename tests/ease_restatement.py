"""NumPy restatement of EASE (include/anirec.h: anirec_spd_inverse, anirec_ease_weights, anirec_ease_scores), fp64.

``spd_inverse`` is the blocked Gauss-Jordan elimination exactly as the header of csrc/anirec_ease.hip defines it, block
step by block step: the diagonal block by the unblocked form of the same elimination, the row panel Rp = R A[K][:], the
update A[I][J] - A[I][K] Rp[:][J], the negated column panel, the diagonal block itself.  NumPy's matmul adds in its own
order and does not fuse, and the matrix cores' order inside an instruction is not documented, so this restatement and
the kernel are held to the same residual, not to each other's bits.  The weights and the score rows are exact rules:
those the kernels match bit for bit.
"""
import numpy as np

from cooc_restatement import unpack_bits

NB = 64                 # anirec_spd_inverse_block()
Q_SCALE = float(1 << 30)
MAX_TERM = 1024.0
NAN32 = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]


def gram_matrix(bits, n_users, reg):
    """A = B B^T + reg I in fp64 from liked-by bit rows (uint32 [n, ceil(n_users/32)])."""
    B = unpack_bits(bits, n_users).astype(np.float64)       # 0 / 1: the sums are exact
    A = B @ B.T
    A[np.diag_indices_from(A)] += float(reg)
    return A


def _invert_block(D):
    """(the inverse of a diagonal block by unblocked Gauss-Jordan in pivot order, whether a pivot failed)"""
    D = D.copy()
    m = len(D)
    fail = False
    with np.errstate(all="ignore"):
        for p in range(m):
            piv = D[p, p]
            if not (piv > 0.0 and np.isfinite(piv)):
                fail = True
            t = 1.0 / piv
            row, col = D[p] * t, D[:, p].copy()
            D -= np.outer(col, row)
            D[p] = row
            D[:, p] = -(col * t)
            D[p, p] = t
    return D, fail


def spd_inverse(A, nb=NB):
    """(the inverse of the symmetric positive definite A, info): info = 0, or 1 + the first block step whose diagonal
    block met a pivot that was not > 0 or not finite."""
    A = np.array(A, np.float64)
    n = len(A)
    info = 0
    with np.errstate(all="ignore"):
        for b, k0 in enumerate(range(0, n, nb)):
            K = slice(k0, min(n, k0 + nb))
            R, fail = _invert_block(A[K, K])
            if fail and not info:
                info = b + 1
            Rp = R @ A[K]                       # the row panel, all columns (those of K are replaced below)
            C = A[:, K].copy()
            A -= C @ Rp
            A[K] = Rp
            A[:, K] = -(C @ R)
            A[K, K] = R
    return A, info


def ease_weights(P):
    """fp32 [n, n]: -P[i][j] / P[j][j] in fp64, rounded once; the diagonal +0."""
    P = np.asarray(P, np.float64)
    with np.errstate(all="ignore"):
        W = (-P / np.diag(P)[None, :]).astype(np.float32)
    W[np.diag_indices_from(W)] = np.float32(0.0)
    return W


def ease_scores(W, offsets, hist_idx, hist_w=None):
    """Returns (out fp32 [n_lists, n_items], err): anirec_itemknn_scores' term rule over the rows of W."""
    W = np.asarray(W, np.float32)
    n = len(W)
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
            with np.errstate(invalid="ignore", over="ignore"):
                prod = w * W[i, :n].astype(np.float64)
                ok = np.abs(prod) <= MAX_TERM               # False for NaN
            if not ok.all():
                err = 1
            S += np.where(ok, np.rint(np.where(ok, prod, 0.0) * Q_SCALE), 0.0).astype(np.int64)
        out[l] = (S.astype(np.float64) * (1.0 / Q_SCALE)).astype(np.float32)
    return out, err


def ease_fit(bits, n_users, reg, nb=NB):
    """W of the liked-by bit rows through the blocked inverse; ValueError when it meets a bad pivot."""
    P, info = spd_inverse(gram_matrix(bits, n_users, reg), nb)
    if info:
        raise ValueError("ease_fit: reg = %r is too small" % reg)
    return ease_weights(P)


def ranks(scores, seen, target_row, target_anime):
    """The rank of every target in its row's order (larger first, ties by index) among the items the row has not seen,
    the target's own seen bit ignored: what rows_rank gives for rows without NaN or signed zeros to tell apart."""
    S = np.asarray(scores, np.float32)
    out = np.empty(len(target_row), np.int64)
    for t, (r, a) in enumerate(zip(target_row, target_anime)):
        cand = ~np.asarray(seen[r], bool)
        cand[a] = False
        s = S[r].astype(np.float64) + 0.0
        out[t] = int(np.sum(cand & ((s > s[a]) | ((s == s[a]) & (np.arange(len(s)) < a)))))
    return out


def residual(A, P):
    """max |A P - I|"""
    return float(np.abs(np.asarray(A) @ np.asarray(P) - np.eye(len(A))).max())
