"""A NumPy restatement of the content-based score rows (include/anirec.h, anirec_content_scores) and of
``recs.content_fit``'s TF-IDF, as the header and the docstring state them:

    Wq   = sum_e rint(|w_e| 2^30)                              int64
    P[v] = sum_e sum_{t in row(i_e), tok[t] == v} rint(w_e x_t 2^30)      int64, the fp64 product of two fp32 exact
    p[v] = Wq > 0 ? fp32(fp64(P[v]) / fp64(Wq)) : 0
    out[l][j] = the chain acc = fma(p[tok[t]], x_t, acc) over item j's slots in storage order, from +0

Integer sums and a fixed chain: nothing here depends on an order, so the GPU result has to equal it bit for bit.  The
chain goes through ``als_restatement.fma_exact``."""
import math
import re
from collections import Counter

import numpy as np

from als_restatement import fma_exact

F32 = np.float32
NAN32 = np.uint32(0x7FC00000).view(np.float32)
SCALE = 2.0 ** 30
MAX_TERM = 1024.0


def _csr(tok_offsets, tok_idx, tok_w):
    return (np.asarray(tok_offsets, np.int64).reshape(-1), np.asarray(tok_idx, np.int64).reshape(-1),
            np.asarray(tok_w, F32).reshape(-1))


def profiles(tok_offsets, tok_idx, tok_w, n_tokens, hist_offsets, hist_idx, hist_w=None):
    """(P int64 [n_lists, n_tokens], Wq int64 [n_lists], valid bool [n_lists], err): the integer profile sums; a list
    with a bad offsets pair is not valid and its sums are 0."""
    to, ti, tw = _csr(tok_offsets, tok_idx, tok_w)
    n = len(to) - 1
    off = np.asarray(hist_offsets, np.int64).reshape(-1)
    hi = np.asarray(hist_idx, np.int64).reshape(-1)
    hw = np.ones(len(hi), F32) if hist_w is None else np.asarray(hist_w, F32).reshape(-1)
    n_l = len(off) - 1
    P, Wq, valid, err = np.zeros((n_l, n_tokens), np.int64), np.zeros(n_l, np.int64), np.ones(n_l, bool), 0
    for l in range(n_l):
        lo, hi_ = int(off[l]), int(off[l + 1])
        if lo < 0 or hi_ < lo or hi_ > len(hi):
            err, valid[l] = 1, False
            continue
        i, w = hi[lo:hi_], hw[lo:hi_].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = (i >= 0) & (i < n) & (np.abs(w) <= MAX_TERM)       # (a NaN fails the comparison)
        if not ok.all():
            err = 1
        i, w = i[ok], w[ok]
        Wq[l] = np.rint(np.abs(w) * SCALE).astype(np.int64).sum()
        cnt = to[i + 1] - to[i]
        slot = np.repeat(to[i] - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
        v, x, ws = ti[slot], tw[slot].astype(np.float64), np.repeat(w, cnt)
        with np.errstate(invalid="ignore", over="ignore"):
            prod = ws * x                                           # exact: two 24-bit significands
            fine = (v >= 0) & (v < n_tokens) & (np.abs(prod) <= MAX_TERM)
        if not fine.all():
            err = 1
        np.add.at(P[l], v[fine], np.rint(prod[fine] * SCALE).astype(np.int64))
    return P, Wq, valid, err


def profile_image(P, Wq):
    """p fp32 [n_lists, n_tokens]: fp32(fp64(P) / fp64(Wq)), 0 where Wq is not positive"""
    out = np.zeros(P.shape, F32)
    pos = Wq > 0
    out[pos] = (P[pos].astype(np.float64) / Wq[pos].astype(np.float64)[:, None]).astype(F32)
    return out


def content_scores(tok_offsets, tok_idx, tok_w, n_tokens, hist_offsets, hist_idx, hist_w=None):
    """Returns (out fp32 [n_lists, n_items], err)."""
    to, ti, tw = _csr(tok_offsets, tok_idx, tok_w)
    n = len(to) - 1
    P, Wq, valid, err = profiles(to, ti, tw, n_tokens, hist_offsets, hist_idx, hist_w)
    p = profile_image(P, Wq)
    usable = (ti >= 0) & (ti < n_tokens) & np.isfinite(tw)
    if valid.any() and not usable.all():
        err = 1
    out = np.zeros((len(valid), n), F32)
    # the chain, a position at a time over the usable slots of every item at once
    rows = [np.arange(to[j], to[j + 1])[usable[to[j]:to[j + 1]]] for j in range(n)]
    length = np.asarray([len(r) for r in rows])
    for t in range(int(length.max()) if n else 0):
        items = np.flatnonzero(length > t)
        slot = np.asarray([rows[j][t] for j in items])
        out[:, items] = fma_exact(p[:, ti[slot]], tw[slot][None, :], out[:, items])
    out[~valid] = NAN32
    return out, err


def ops_content_scores(tok_offsets, tok_idx, tok_w, n_tokens, hist_offsets, hist_idx, hist_w=None):
    out, err = content_scores(tok_offsets, tok_idx, tok_w, n_tokens, hist_offsets, hist_idx, hist_w)
    if err:
        raise ValueError("content_scores: out of range")
    return out


# ---- content_fit's TF-IDF -------------------------------------------------------------------------------------------
def tfidf(cells_by_column, min_df=1, max_df=1.0, synopsis="Sypnopsis"):
    """(vocab, tok_offsets int64, tok_idx int32, tok_w fp32) of ``recs.content_fit``: ``cells_by_column`` maps a column to
    its list of cells, in the order the columns are given."""
    n = len(next(iter(cells_by_column.values())))
    tf = [{} for _ in range(n)]
    for col, cells in cells_by_column.items():
        if col == synopsis:
            counts = [Counter(re.findall(r"[a-z]{3,}", c.lower())) if isinstance(c, str) and c != "None" else Counter()
                      for c in cells]
            df = Counter(t for c in counts for t in c)
            for row, c in zip(tf, counts):
                for t, k in c.items():
                    if min_df <= df[t] <= max_df * n:
                        row[col + "=" + t] = 1.0 + math.log(k)
        else:
            for row, c in zip(tf, cells):
                if isinstance(c, str):
                    for t in c.split(","):
                        if t.strip():
                            row[col + "=" + t.strip()] = 1.0
    vocab = sorted({t for row in tf for t in row})
    df = Counter(t for row in tf for t in row)
    off, idx, w = [0], [], []
    for row in tf:
        toks = [t for t in vocab if t in row]
        raw = [row[t] * (math.log((1.0 + n) / (1.0 + df[t])) + 1.0) for t in toks]
        norm = math.sqrt(math.fsum(x * x for x in raw))
        idx += [vocab.index(t) for t in toks]
        w += [x / norm for x in raw]
        off.append(len(idx))
    return vocab, np.asarray(off, np.int64), np.asarray(idx, np.int32), np.asarray(w, np.float32)
