"""A NumPy restatement of the bootstrap entry points (include/anirec.h: anirec_rank_gain_rows, anirec_boot_sums,
anirec_boot_weights), written from the definition and nothing else.  A plain helper module, imported by
the tests the way ``cooc_restatement`` is.

The statistic: the resampling unit is the user; replicate b >= 1 gives the unit with key ``key`` the integer weight
    mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16        (uint32, mod 2**32)
    r = mix32( mix32(seed + 0x9e3779b9 * b) ^ mix32(key + 0x85ebca6b) )
    w = #{ j < n_thr : r >= thr[j] }
and replicate 0 the weight 1.  With thr[j] = floor(2**32 * CDF(j)) of Poisson(1) the weights are Poisson(1) draws.
Sums are int64 and exact."""
from decimal import Decimal, getcontext

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
MAX_THR = 16


def _u(x):
    """Anything integer, reduced mod 2**32, as uint64 (so products do not overflow before the mask)."""
    return (np.asarray(x).astype(np.int64) & np.int64(0xFFFFFFFF)).astype(np.uint64)


def mix32(x):
    x = _u(x)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def draw(seed, b, key):
    """r(seed, b, key) as uint32; ``b`` and ``key`` broadcast."""
    hb = mix32((_u(seed) + np.uint64(0x9e3779b9) * _u(b)) & M32)
    hk = mix32((_u(key) + np.uint64(0x85ebca6b)) & M32)
    return mix32(hb ^ hk).astype(np.uint32)


def check_thr(thr):
    t = [int(x) for x in thr]
    ok = len(t) <= MAX_THR and all(0 <= x <= 0xFFFFFFFF for x in t) and all(a <= b for a, b in zip(t, t[1:]))
    return t if ok else None


def weight(r, thr):
    r = np.asarray(r, np.uint32)
    w = np.zeros(r.shape, np.uint8)
    for t in thr:
        w += r >= np.uint32(t)
    return w


def boot_weights(keys, seed, n_rep, thr):
    """uint8 [n_rep, n_units]: row b - 1 the weights of replicate b = 1 .. n_rep."""
    keys = np.asarray(keys).reshape(-1)
    b = np.arange(1, n_rep + 1, dtype=np.int64)[:, None]
    return weight(draw(seed, b, keys[None, :]), thr).reshape(n_rep, keys.size)


def poisson1_thresholds(n=13):
    """floor(2**32 * CDF(j)) of Poisson(1), j = 0 .. n - 1, from 60-digit decimals."""
    getcontext().prec = 60
    e_inv = Decimal(-1).exp()
    out, cdf, term = [], Decimal(0), Decimal(1)
    for j in range(n):
        if j:
            term /= j
        cdf += term * e_inv
        out.append(int(cdf * (1 << 32)))
    return out


def boot_limit(n_units, n_thr):
    return (1 << 62) // (max(n_thr, 1) * max(n_units, 1))


def rank_gain_rows(ranks, target_unit, n_units, gain):
    """(out int64 [n_units, n_sys * n_metric + 1], err): the literal loops."""
    ranks = np.asarray(ranks, np.int64)
    gain = np.asarray(gain).astype(np.int64)
    unit = np.asarray(target_unit, np.int64).reshape(-1)
    n_sys, n_metric, n_gain = ranks.shape[0], gain.shape[0], gain.shape[1]
    out = np.zeros((n_units, n_sys * n_metric + 1), np.int64)
    ok = (unit >= 0) & (unit < n_units)
    for s in range(n_sys):
        r = ranks[s][ok]
        inside = (r >= 0) & (r < n_gain)
        for m in range(n_metric):
            g = np.where(inside, gain[m][np.where(inside, r, 0)], 0)
            np.add.at(out[:, s * n_metric + m], unit[ok], g)
    np.add.at(out[:, -1], unit[ok], 1)
    return out, int(not ok.all())


def boot_sums(values, keys, seed, n_rep, thr):
    """(out int64 [n_rep + 1, n_col], err): row 0 the column sums, row b the sums under replicate b's weights; all -1 and
    err = 1 when a value lies outside [0, boot_limit)."""
    v = np.asarray(values, np.int64)
    keys = np.asarray(keys).reshape(-1)
    n_units, n_col = v.shape
    if n_units and ((v < 0) | (v >= boot_limit(n_units, len(thr)))).any():
        return np.full((n_rep + 1, n_col), -1, np.int64), 1
    W = np.concatenate([np.ones((1, n_units), np.int64), boot_weights(keys, seed, n_rep, thr).astype(np.int64)])
    return W @ v if n_units else np.zeros((n_rep + 1, n_col), np.int64), 0


# ---- the wrappers of ops, on CPU tensors -----------------------------------------------------------------------------
def _n(x):
    import torch
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def ops_rank_gain_rows(ranks, target_unit, n_units, gain, check=True):
    import torch
    g = _n(gain).astype(np.int64) & 0xFFFFFFFF
    out, err = rank_gain_rows(_n(ranks), _n(target_unit), int(n_units), g)
    if not check:
        return torch.as_tensor(out), torch.as_tensor([err], dtype=torch.int32)
    if err:
        raise ValueError("rank_gain_rows: target_unit out of range")
    return torch.as_tensor(out)


def ops_boot_sums(values, unit_key, seed, n_rep, thr, workspace=None, check=True):
    import torch
    t = check_thr(thr)
    if t is None or not 0 <= int(n_rep) <= 65536:
        raise ValueError("bootstrap: bad n_rep or threshold table")
    out, err = boot_sums(_n(values), _n(unit_key), int(seed), int(n_rep), t)
    if not check:
        return torch.as_tensor(out), torch.as_tensor([err], dtype=torch.int32)
    if err:
        raise ValueError("boot_sums: a value is negative or too large")
    return torch.as_tensor(out)


def ops_boot_weights(unit_key, seed, n_rep, thr, device=None):
    import torch
    return torch.as_tensor(boot_weights(_n(unit_key), int(seed), int(n_rep), check_thr(thr)))
