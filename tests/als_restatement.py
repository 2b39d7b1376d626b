"""NumPy restatement of implicit-feedback ALS (include/anirec.h, anirec_als_gram / anirec_als_half_sweep; DESIGN.md
4.17): the definition in fp64, and the same in fp32 in the kernel's documented order.  A plain helper module, imported by
the tests the way ``foldin_restatement`` is.

    A v       G v + lambda v + sum_k e_k (y_k . v) y_k                                 (never formed as a matrix)
    empty     x = 0 exactly, row_loss = 0, no iteration
    start     r = sum_k ((1 + e_k) - e_k (y_k . x)) y_k - G x - lambda x;  p = r;  rs0 = rs = r . r
    step      stop unless rs > RTOL2 rs0;  a = rs / (p . Ap);  x += a p;  r -= a Ap;  rs' = r . r;
              p = r + (rs' / rs) p;  rs = rs'
    row_loss  x . G x + sum_k [(1 + e_k)(1 - s_k)^2 - s_k^2] + lambda x . x,  s_k = y_k . x

fp32 order (``half_sweep32``): kNG = 1024 / F lane groups of F / 4 lanes, lane l holding elements 4l .. 4l+3.
    u . v     per lane ((u0 v0 + u1 v1) + u2 v2) + u3 v3, then the xor butterfly over the lanes at distances F/8 .. 1
    a walk    group g starts from 0, adds w_k G[k] for k = g, g + kNG, .. (w_k = v[k]; -v[k] in the start residual),
              then c_k y_k for the entries k = g, g + kNG, .. in list order; the partial rows are added in group order;
              the lambda term last
    row_loss  (x . Gx + L) + lambda (x . x)
Every product and sum is rounded once: NumPy float32 arrays never fuse.

Every executed step asserts rs / (RTOL2 rs0) >= EXIT_MARGIN, so that no fp32 / fp64 pair can take different exits.
"""
import numpy as np

RTOL2 = 1e-10           # ANIREC_ALS_CG_RTOL2
MAX_CG = 16             # ANIREC_ALS_MAX_CG
EXIT_MARGIN = 1e3
F32 = np.float32


def gram64(Y):
    Y = np.asarray(Y, np.float64)
    return Y.T @ Y


def gram_bound(Y):
    """The header's bound on |anirec_als_gram - gram64|: 2^-24 |G64| + n 2^-52 sum_r |Y[r][a] Y[r][b]|"""
    Y = np.asarray(Y, np.float64)
    return 2.0 ** -24 * np.abs(Y.T @ Y) + Y.shape[0] * 2.0 ** -52 * (np.abs(Y).T @ np.abs(Y))


def row_lists(offsets, idx, excess, alpha, dtype):
    """[(idx int64 [n], e dtype [n])] per row; ``excess`` None means ``alpha`` for every entry"""
    off = np.asarray(offsets, np.int64)
    idx = np.asarray(idx, np.int64)
    out = []
    for u in range(len(off) - 1):
        i = idx[off[u]:off[u + 1]]
        e = np.full(len(i), alpha, dtype) if excess is None else np.asarray(excess, dtype)[off[u]:off[u + 1]]
        out.append((i, e))
    return out


def normal_equations(Y, i, e, lam):
    """(A, b) of one row, explicitly, in fp64"""
    Y = np.asarray(Y, np.float64)
    e = np.asarray(e, np.float64)
    Yi = Y[i]
    A = Y.T @ Y + (Yi * e[:, None]).T @ Yi + lam * np.eye(Y.shape[1])
    return A, ((1.0 + e)[:, None] * Yi).sum(0)


def objective_brute(Y, i, e, lam, x):
    """The row's share of the objective summed over ALL items in fp64 (a list without repeats): confidence 1 + e and
    preference 1 on the list, 1 and 0 off it"""
    Y = np.asarray(Y, np.float64)
    assert len(set(np.asarray(i).tolist())) == len(i)
    c = np.ones(len(Y))
    p = np.zeros(len(Y))
    c[i] += np.asarray(e, np.float64)
    p[i] = 1.0
    return float((c * (p - Y @ x) ** 2).sum() + lam * (x @ x))


def row64(Y, G, i, e, lam, x, cg_steps, margins=None, rtol2=RTOL2):
    """One row in fp64.  Returns (x, row_loss).  ``rtol2`` other than the definition's is for the convergence
    test alone (1e-30: as far as fp64 goes) and checks no margin."""
    Y, G = np.asarray(Y, np.float64), np.asarray(G, np.float64)
    e = np.asarray(e, np.float64)
    x = np.asarray(x, np.float64).copy()
    if len(i) == 0:
        return np.zeros_like(x), 0.0
    Yi = Y[i]

    def A(v):
        return G @ v + lam * v + Yi.T @ (e * (Yi @ v))
    if cg_steps > 0:
        r = Yi.T @ ((1.0 + e) - e * (Yi @ x)) - (G @ x + lam * x)
        p = r.copy()
        rs0 = rs = r @ r
        for _ in range(cg_steps):
            if not rs > rtol2 * rs0:
                break
            if rtol2 == RTOL2:
                _margin(rs, rs0, margins)
            Ap = A(p)
            a = rs / (p @ Ap)
            x += a * p
            r -= a * Ap
            rsn = r @ r
            p = r + (rsn / rs) * p
            rs = rsn
    s = Yi @ x
    return x, float(x @ (G @ x) + ((1.0 + e) * (1.0 - s) ** 2 - s ** 2).sum() + lam * (x @ x))


def _margin(rs, rs0, margins):
    m = float(rs) / (RTOL2 * float(rs0))
    assert m >= EXIT_MARGIN, "a step runs %g above the exit: change the case, not the margin" % m
    if margins is not None:
        margins.append(m)


def _gsum32(a):
    """the xor butterfly over the last axis (the lanes of a group); every lane ends with the same bits"""
    kG = a.shape[-1]
    lanes = np.arange(kG)
    o = kG // 2
    while o >= 1:
        a = a + a[..., lanes ^ o]
        o //= 2
    return a[..., 0]


def _dot32(U, v):
    """U [..., F] . v [F] in the kernel's order"""
    F = v.shape[-1]
    p = U.reshape(U.shape[:-1] + (F // 4, 4)) * v.reshape(F // 4, 4)
    return _gsum32(((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])


def _walk32(mode, Y, G, i, e, v):
    """mode 0: A v without lambda; 1: the start residual without lambda; 2: (G v, the loss sum).  fp32 throughout."""
    F = v.shape[0]
    kNG = 1024 // F
    acc = np.zeros((kNG, F), F32)
    w = -v if mode == 1 else v
    for k0 in range(0, F, kNG):
        acc = acc + w[k0:k0 + kNG, None] * G[k0:k0 + kNG]
    Yi = Y[i]
    s = _dot32(Yi, v)
    one = F32(1)
    lsum = np.zeros(kNG, F32)
    if mode == 2:
        d = one - s
        term = (one + e) * (d * d) - s * s
    else:
        c = (one + e) - e * s if mode == 1 else e * s
    for k0 in range(0, len(i), kNG):
        m = min(kNG, len(i) - k0)
        if mode == 2:
            lsum[:m] = lsum[:m] + term[k0:k0 + m]
        else:
            acc[:m] = acc[:m] + c[k0:k0 + m, None] * Yi[k0:k0 + m]
    t, lt = acc[0], lsum[0]
    for g in range(1, kNG):
        t = t + acc[g]
        lt = lt + lsum[g]
    return t, lt


def row32(Y, G, i, e, lam, x, cg_steps, margins=None):
    """One row in fp32 in the kernel's order.  Returns (x fp32, row_loss fp32)."""
    Y, G = np.asarray(Y, F32), np.asarray(G, F32)
    e = np.asarray(e, F32)
    x = np.asarray(x, F32).copy()
    lam = F32(lam)
    if len(i) == 0:
        return np.zeros_like(x), F32(0)
    if cg_steps > 0:
        r, _ = _walk32(1, Y, G, i, e, x)
        r = r - lam * x
        p = r.copy()
        rs = _dot32(r, r)
        rs0 = rs
        floor = F32(RTOL2) * rs0
        for _ in range(cg_steps):
            if not rs > floor:
                break
            _margin(rs, rs0, margins)
            Ap, _ = _walk32(0, Y, G, i, e, p)
            Ap = Ap + lam * p
            a = rs / _dot32(p, Ap)
            x = x + a * p
            r = r - a * Ap
            rsn = _dot32(r, r)
            p = r + (rsn / rs) * p
            rs = rsn
    Gx, lt = _walk32(2, Y, G, i, e, x)
    return x, (_dot32(x, Gx) + lt) + lam * _dot32(x, x)


def half_sweep(Y, G, offsets, idx, excess, alpha, X, lam, cg_steps, dtype=np.float64, margins=None):
    """Every row of X refitted against Y and G.  Returns (X dtype [n_rows, F], row_loss dtype [n_rows])."""
    assert 0 <= cg_steps <= MAX_CG
    one = row64 if dtype == np.float64 else row32
    X = np.asarray(X, dtype)
    out, loss = np.empty_like(X), np.empty(len(X), dtype)
    for u, (i, e) in enumerate(row_lists(offsets, idx, excess, alpha, dtype)):
        out[u], loss[u] = one(Y, G, i, e, lam, X[u], cg_steps, margins)
    return out, loss


def csr(row, col, n_rows, weight=None):
    """A stable sort by row: (offsets int64, col in the pairs' own order per row, weight likewise or None)"""
    row = np.asarray(row, np.int64)
    order = np.argsort(row, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n_rows))]).astype(np.int64)
    return off, np.asarray(col, np.int64)[order], None if weight is None else np.asarray(weight)[order]


def init_tables(n_users, n_items, factors, seed):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n_users, factors)) * 0.01).astype(F32)
    Y = (rng.standard_normal((n_items, factors)) * 0.01).astype(F32)
    return X, Y


def fit(user_idx, item_idx, n_users, n_items, factors, sweeps, cg_steps, alpha, reg, weight=None, seed=0,
        dtype=np.float64):
    """``recs.als_fit`` driven the same way: users then items per sweep, G recomputed before each half (the fp64 Gram
    rounded once to ``dtype``), the loss after every half-sweep = the row losses summed in fp64 + reg |frozen table|^2.
    Returns (X, Y, losses)."""
    X, Y = (t.astype(dtype) for t in init_tables(n_users, n_items, factors, seed))
    ex = None if weight is None else (F32(alpha) * np.asarray(weight, F32))
    u_off, u_idx, u_ex = csr(user_idx, item_idx, n_users, ex)
    i_off, i_idx, i_ex = csr(item_idx, user_idx, n_items, ex)
    losses = []
    for _ in range(sweeps):
        X, rl = half_sweep(Y, gram64(Y).astype(dtype), u_off, u_idx, u_ex, alpha, X, reg, cg_steps, dtype)
        losses.append(float(rl.astype(np.float64).sum() + reg * (Y.astype(np.float64) ** 2).sum()))
        Y, rl = half_sweep(X, gram64(X).astype(dtype), i_off, i_idx, i_ex, alpha, Y, reg, cg_steps, dtype)
        losses.append(float(rl.astype(np.float64).sum() + reg * (X.astype(np.float64) ** 2).sum()))
    return X, Y, losses


def dot_chain(Q, Y):
    """out[q][j] = the chain acc = fmaf(Q[q][t], Y[j][t], acc) over t in index order, from 0: a float32 product is
    exact in float64 and the float64 sum of it and a float32 is rounded to float32 — a double rounding that differs from
    the fused one only when the float64 sum lands exactly on a float32 tie, which ``fma_exact`` (below) settles."""
    Q, Y = np.asarray(Q, F32), np.asarray(Y, F32)
    acc = np.zeros((len(Q), len(Y)), F32)
    for t in range(Q.shape[1]):
        acc = fma_exact(Q[:, t][:, None], Y[:, t][None, :], acc)
    return acc


def fma_exact(a, b, c):
    """float32 fma(a, b, c), exactly: the product p is exact in float64; s = p + c in float64 with the rounding error
    recovered by TwoSum; where s is a float32 tie the error's sign breaks it as the infinitely precise sum would"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    out = s.astype(F32)
    # a tie: s lies exactly halfway between two neighbouring floats, and the exact sum lies to one side of it
    lo = np.nextafter(out, F32(-np.inf)).astype(np.float64)
    hi = np.nextafter(out, F32(np.inf)).astype(np.float64)
    o64 = out.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tie_up = (s - o64 == (hi - o64) / 2) & (err > 0) & (s > o64)      # rounded down to even, the sum is above the tie
        tie_dn = (o64 - s == (o64 - lo) / 2) & (err < 0) & (s < o64)      # rounded up to even, the sum is below the tie
    out = np.where(tie_up, hi.astype(F32), out)
    out = np.where(tie_dn, lo.astype(F32), out)
    return out
