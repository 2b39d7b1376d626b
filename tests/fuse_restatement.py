"""The definition of anirec_fuse_rows (include/anirec.h) in NumPy: the yardstick of the fusion tests.

The order of a row is the select's: ``score_key`` (restated on uint32 views in cooc_restatement) descending, ties to the
ascending index; ranks come from ``np.lexsort`` on (index, key).  Every fp32 step is a ``np.float32`` operation in the
stated order — one division per term, one add per system — so the kernel is held to these bits exactly."""
import numpy as np

from cooc_restatement import score_key, unpack_bits

RRF, MINMAX = 0, 1
METHODS = {"rrf": RRF, "minmax": MINMAX}
MAX_SYS = 8
MAX_ITEMS = 20480
MAX_RRF_C = 1 << 20
NAN_BITS = np.uint32(0x7FC00000)
NAN32 = np.array([NAN_BITS], np.uint32).view(np.float32)[0]


def eligible(nq, n, wbits=None, keep=None):
    """bool [nq, n]: keep[j] != 0 and the watched bit clear (bits at positions >= n are ignored)"""
    E = np.ones((nq, n), bool)
    if keep is not None:
        E &= (np.asarray(keep).reshape(-1)[:n] != 0)[None, :]
    if wbits is not None:
        E &= ~unpack_bits(np.ascontiguousarray(wbits).view(np.uint32).reshape(nq, -1), n)
    return E


def _row(x, t, n):
    x = np.asarray(x, np.float32)
    return x[:n] if x.ndim == 1 else x[t, :n]


def ranks(x, e):
    """int64 [n]: the 0-based place of every eligible item among the eligible items (-1 elsewhere)"""
    j = np.flatnonzero(e)
    key = score_key(x[j]).astype(np.int64)
    order = np.lexsort((j, -key))
    r = np.full(len(x), -1, np.int64)
    r[j[order]] = np.arange(len(j))
    return r


def rrf_terms(x, e, w, c):
    r = ranks(x, e)
    t = np.zeros(len(x), np.float32)
    t[e] = np.float32(w) / (np.int64(c) + 1 + r[e]).astype(np.float32)
    return t


def minmax_terms(x, e, w):
    key = score_key(x)
    fin = e & np.isfinite(x)
    v = np.zeros(len(x), np.float32)
    with np.errstate(all="ignore"):
        if fin.any():
            j = np.flatnonzero(fin)
            hi, lo = x[j[np.argmax(key[j])]], x[j[np.argmin(key[j])]]
            span = np.float32(hi - lo)
            if span != 0:
                q = ((x[fin] - lo).astype(np.float32) / span).astype(np.float32)
                q[np.isnan(q)] = NAN32                   # inf / inf where hi - lo overflows: the canonical NaN
                v[fin] = q
        v[e & (x == np.inf)] = np.float32(1.0)
        return (np.float32(w) * v).astype(np.float32)


def fuse_rows(rows, weights=None, method=RRF, rrf_c=60, n=None, wbits=None, keep=None, nq=None):
    """fp32 [nq, n]: the fused value of an eligible item, the canonical NaN elsewhere.  ``rows``: fp32 [nq, ld] arrays or
    1-D vectors shared by every row."""
    rows = [np.asarray(r, np.float32) for r in rows]
    n = min(r.shape[-1] for r in rows) if n is None else int(n)
    if nq is None:
        two = [r for r in rows if r.ndim == 2]
        nq = two[0].shape[0] if two else (1 if wbits is None else np.asarray(wbits).shape[0])
    w = np.ones(len(rows), np.float32) if weights is None else np.asarray(weights, np.float32)
    E = eligible(nq, n, wbits, keep)
    out = np.full((nq, n), NAN32, np.float32)
    for t in range(nq):
        e = E[t]
        acc = np.zeros(n, np.float32)
        for s, r in enumerate(rows):
            x = _row(r, t, n)
            term = rrf_terms(x, e, w[s], rrf_c) if method == RRF else minmax_terms(x, e, w[s])
            with np.errstate(all="ignore"):
                acc = (acc + term).astype(np.float32)
        out[t, e] = acc[e]
    return out


# ---- the wrapper's signature on NumPy arrays (tests that run host logic with ``ops`` replaced) ------------------------
def ops_fuse_rows(rows, weights=None, method="rrf", rrf_c=60, n=None, wbits=None, keep=None):
    from anime_recommendations_amd import ops
    rows = [np.asarray(r, np.float32) for r in rows]
    n = min(r.shape[-1] for r in rows) if n is None else n
    _, n, ws, m, c = ops.check_fuse(len(rows), n, weights, method, rrf_c)
    return fuse_rows(rows, ws, m, c, n, wbits, keep)
