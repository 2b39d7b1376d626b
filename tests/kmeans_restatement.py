"""NumPy restatement of the clustered tables (include/anirec.h, anirec_kmeans_assign / anirec_kmeans_fit): the
definition of the header comment, step for step.  The assign rule works on a GIVEN similarity matrix (the chain's bits
come from code that is not under test), the update rule on ``What`` itself.  A plain helper module, imported by the tests
the way ``explain_restatement`` is.

    usable   every element of the row finite and |x| <= 2
    pick     the centroids in ascending c: a NaN sim is never taken, the first pickable one is, a later one only when
             strictly larger (ties, -0 == +0 among them, stay with the lowest c); +-inf are ordinary numbers;
             -1 / NaN (0x7FC00000) for an unusable row and for a row without a pickable centroid
    q(x)     np.rint(float64(x) * 2**30) as int64: an exact product, rounded to the nearest even integer
    S_c[t]   the int64 sum of q over the rows assigned to c
    update   d = float64(S_c); nn = the chain over ascending t of nn + d[t] * d[t], each product and each sum rounded
             (NumPy float64 scalars never fuse); nn > 0: C[c] = float32(d / sqrt(nn)); otherwise the bits are kept
    fit      a_0 = -2; iteration j: assign, changed_j, stop at 0 (C untouched), else update; after max_iter iterations
             without a stop one more assign with the final C
"""
import numpy as np

NAN32 = np.float32(np.nan)
Q_SCALE = float(2 ** 30)


def usable(What):
    """bool [n]: every element finite and at most 2 in magnitude (a NaN fails the comparison)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(What, np.float32)) <= np.float32(2)).all(axis=1)


def assign(S, ok):
    """``S`` [n, k] fp32: S[i, c] = sim(i, c); ``ok`` [n] bool: the usable rows.  Returns (assign int32 [n], sim fp32 [n])."""
    S = np.asarray(S, np.float32)
    n, k = S.shape
    best = np.full(n, NAN32, np.float32)
    bc = np.full(n, -1, np.int32)
    with np.errstate(invalid="ignore"):
        for c in range(k):
            s = S[:, c]
            take = ~np.isnan(s) & ((bc < 0) | (s > best))
            best[take] = s[take]
            bc[take] = c
    bad = ~np.asarray(ok, bool)
    bc[bad] = -1
    best[bad] = NAN32
    return bc, best


def quantise(What):
    """q of every element, int64 (the rows a fit uses are usable: finite, |x| <= 2)."""
    return np.rint(np.asarray(What, np.float32).astype(np.float64) * Q_SCALE).astype(np.int64)


def update(What, a, C):
    """The centroids after one update: ``a`` [n] the assignment (-1 = none), ``C`` [k, dim] fp32 the current centroids.
    Returns (C_new fp32 [k, dim], count int32 [k])."""
    C = np.array(C, np.float32, copy=True)
    k, dim = C.shape
    a = np.asarray(a)
    used = np.flatnonzero(a >= 0)
    S = np.zeros((k, dim), np.int64)
    np.add.at(S, a[used], quantise(np.asarray(What)[used]))
    count = np.bincount(a[used], minlength=k).astype(np.int32)
    d = S.astype(np.float64)
    nn = np.zeros(k, np.float64)
    for t in range(dim):                                    # one rounded product, one rounded sum a step
        nn = nn + d[:, t] * d[:, t]
    for c in range(k):
        if count[c] > 0 and nn[c] > 0:
            C[c] = (d[c] / np.sqrt(nn[c])).astype(np.float32)
    return C, count


def fit(What, C0, max_iter, sims):
    """The fit loop.  ``sims(C)`` returns the [n, k] fp32 similarity matrix of ``What`` against the centroids ``C``.
    Returns (C, assign, sim, count, (iterations run, converged))."""
    What = np.asarray(What, np.float32)
    C = np.array(C0, np.float32, copy=True)
    ok = usable(What)
    prev = np.full(len(What), -2, np.int32)
    for j in range(1, int(max_iter) + 1):
        a, s = assign(sims(C), ok)
        if int((a != prev).sum()) == 0:
            return C, a, s, _count(a, len(C)), (j, 1)
        C, _ = update(What, a, C)
        prev = a
    a, s = assign(sims(C), ok)
    return C, a, s, _count(a, len(C)), (int(max_iter), 0)


def _count(a, k):
    return np.bincount(a[a >= 0], minlength=k).astype(np.int32)
