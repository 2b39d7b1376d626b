"""NumPy restatement of the fp16 MFMA screening of the fast inference paths, and constructors of unit rows on which
its error window binds (test infrastructure, shared by tests/test_mfma_bounds_cpu.py and tests/test_mfma_bounds_gpu.py).

What it restates (anirec_topk_mfma.hip, anirec_predict_mfma.hip):
  * the operands: ``k_to_f16`` (RNE of the fp32 row), ``k_norm_f16`` (fp32 l2-normalise, times ``sign``, RNE) and
    ``k_norm_split`` (x 2^8, hi = f16(v), lo = f16(v - hi)); ``np.float16`` rounds to nearest even, as the kernels do;
  * the screening score: the fp16 products summed EXACTLY (fp64: a product of two fp16 values has 22 significant bits,
    a sum of 128 of them fits fp64 without rounding).  The hardware's fp32 accumulation may differ from this by at
    most the kernel's own accumulation term, ``ACC`` = 2 x 128 x 2^-24 = 1.6e-5 — every margin the tests rely on
    exceeds 3 ACC;
  * the selection rule: the k_eff-th largest screening score as an order-preserving key with its low ``SEL_LOW`` bits
    cleared (``f2key`` / the radix select that stops early), the window ``tau - 2 eps``, and the model_recs bound
    ``p_bound = rating_bound(rating(sign (lo + eps)))``.  ``eps`` is a parameter: a test shows what a smaller window
    would lose.

The constructors plant, for one query q, k - 1 anchors well above a level L, a key M at L whose screening score is
understated and a key O just below M in exact score whose screening score is overstated: O becomes tau and M sits
about one eps above the window's lower edge instead of the ~2 eps that random rows leave.  Each designed component
lies ``MID_MARGIN`` (0.1) fp16 half-ulps off its rounding midpoint, on the side that gives the wanted error, so that
the fp32 normalisation of k_norm_f16 (a relative change of ~1e-7 on these unit rows) cannot flip it.
"""
import numpy as np

DIM = 128
EPS = float(np.float32(0.00101))      # kEpsMfma
SEL_LOW = 12                          # kSelLow
UNNORM_TOL = 1e-3                     # k_to_f16: | sum x^2 - 1 | > 1e-3 -> every query to the exact path
ACC = 2 * 128 * 2.0 ** -24            # the two fp32 accumulations of kEpsMfma's derivation
MID_MARGIN = 0.1                      # designed components: this many fp16 half-ulps clear of the rounding midpoint
F16_MIN_NORMAL = 2.0 ** -14
ACTS = ("sigmoid", "linear", "tanh", "relu", "softplus")

f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------
def k_to_f16(W):
    return np.asarray(W, f32).astype(np.float16)


def _rownorm_f32(W):
    """tf l2_normalize in fp32: x * (1 / sqrt(max(sum x^2, 1e-12)))"""
    W = np.asarray(W, f32)
    ss = np.sum(W * W, axis=1, dtype=f32)
    rinv = f32(1) / np.sqrt(np.maximum(ss, f32(1e-12)))
    return W * rinv[:, None], rinv


def k_norm_f16(W, sign=1.0):
    y, _ = _rownorm_f32(W)
    return (y * f32(sign)).astype(np.float16)


def k_norm_split(W):
    """(hi, lo) fp16 planes of 2^8 x the normalised row"""
    W = np.asarray(W, f32)
    ss = np.sum(W * W, axis=1, dtype=f32)
    v = W * (f32(256) / np.sqrt(np.maximum(ss, f32(1e-12))))[:, None]
    hi = v.astype(np.float16)
    lo = (v - hi.astype(f32)).astype(np.float16)
    return hi, lo


def screen(Qh, Kh):
    """fp16 products summed exactly: [nq, nk] fp64"""
    return np.asarray(Qh, np.float64) @ np.asarray(Kh, np.float64).T


def exact(Q, K):
    return np.asarray(Q, np.float64) @ np.asarray(K, np.float64).T


def unnorm_flag(W):
    """k_to_f16's test (fp32 sum of squares)"""
    W = np.asarray(W, f32)
    return bool((np.abs(np.sum(W * W, axis=1, dtype=f32) - f32(1)) > f32(UNNORM_TOL)).any())


# ---------------------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------------------
def f2key(s):
    u = np.asarray(s, f32).view(np.uint32).copy()
    neg = (u & np.uint32(0x80000000)) != 0
    u = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    u[np.isnan(np.asarray(s, f32))] = 0
    return np.where(u == 0, np.uint32(1), u).astype(np.uint32)


def key2f(u):
    u = np.asarray(u, np.uint32)
    b = np.where((u & np.uint32(0x80000000)) != 0, u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32)
    return b.view(f32)


def tau_trunc(m_row, k_eff):
    """the radix select of k_refresh / k_rerank: the k_eff-th largest key with its low SEL_LOW bits cleared"""
    u = np.sort(f2key(np.asarray(m_row, f32)))[::-1]
    kth = u[min(k_eff, len(u)) - 1]
    return f32(key2f(kth & ~np.uint32((1 << SEL_LOW) - 1)))


def window(m_row, k_eff, eps=EPS):
    """(tau, lo, kept mask) of one row: kept = screening score >= tau - 2 eps (fp32, as k_rerank computes lo)"""
    m32 = np.asarray(m_row, f32)
    tau = tau_trunc(m32, k_eff)
    lo = f32(tau - f32(2.0) * f32(eps))
    return tau, lo, m32 >= lo


def act64(name, y):
    y = np.asarray(y, np.float64)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-y))
    if name == "linear":
        return y
    if name == "tanh":
        return np.tanh(y)
    if name == "relu":
        return np.maximum(y, 0.0)
    if name == "softplus":
        return np.logaddexp(0.0, y)
    raise ValueError(name)


ACT_SLACK = {"sigmoid": 6e-7, "linear": 0.0, "relu": 0.0, "tanh": 1e-6, "softplus": 2e-6}   # rating_bound's factors


def rating_bound(name, r):
    r = np.asarray(r, np.float64)
    if name == "sigmoid":
        return r * (1 + ACT_SLACK[name])
    return r + np.abs(r) * ACT_SLACK[name]


def p_bound(lo, eps, sign, hs, hb, act):
    """the best rating a key outside the window can have: rating_bound(rating(sign (lo + eps)))"""
    c = f32(sign) * f32(f32(lo) + f32(eps))
    return rating_bound(act, act64(act, float(c) * hs + hb))


def head_fold(head):
    """(hs, hb) of the BN-inference head, fp32 as the library folds it (anirec_predict_mfma.hip, head_affine_mfma,
    without the 2^-16 of the operand scaling)"""
    inv = f32(f32(1) / np.sqrt(f32(head["mov_var"]) + f32(1e-3))) * f32(head["gamma"])
    hs = f32(f32(head["w"]) * inv)
    hb = f32(f32(head["b"]) * inv + f32(f32(head["beta"]) - f32(head["mov_mean"]) * inv))
    return float(hs), float(hb)


# ---------------------------------------------------------------------------------------------------------------
# constructors
# ---------------------------------------------------------------------------------------------------------------
def _up(g):
    """spacing of the fp16 grid above g > 0"""
    g = np.float16(g)
    return float(np.nextafter(g, np.float16(np.inf))) - float(g)


def _down(g):
    g = np.float16(g)
    return float(g) - float(np.nextafter(g, np.float16(0)))


def rounds_down_from(g):
    """a value above the fp16 value g > 0 that rounds back to g: MID_MARGIN half-ulps short of the midpoint"""
    return float(g) + (1 - MID_MARGIN) * 0.5 * _up(g)


def rounds_up_to(g):
    """a value below the fp16 value g > 0 that rounds up to g"""
    return float(g) - (1 - MID_MARGIN) * 0.5 * _down(g)


def midpoint_clearance(x):
    """distance of each component from its nearest fp16 rounding midpoint, in half-ulps of the grid there"""
    x = np.abs(np.asarray(x, np.float64))
    g = x.astype(np.float16).astype(np.float64)
    up = np.nextafter(g.astype(np.float16), np.float16(np.inf)).astype(np.float64) - g
    dn = g - np.nextafter(g.astype(np.float16), np.float16(0)).astype(np.float64)
    half = np.where(x >= g, up, dn) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(half > 0, np.abs(half - np.abs(x - g)) / half, np.inf)


def _balance(row, dim):
    """set row[dim] so that the row's fp64 squared norm is 1 (the dim carries no designed component)"""
    row[dim] = 0.0
    rest = float(np.sum(row.astype(np.float64) ** 2))
    assert rest < 1.0, rest
    row[dim] = np.sqrt(1.0 - rest)
    return row


# designed frame.  q: A (32 components just above 0.125, rounding down), B (31 just below 0.125 + 2^-13, rounding up),
# QX (one more rounding up) and QF (free: makes the norm 1).  M lies on A (rounding down: both factors of every product
# understated), O on B + QX (rounding up: overstated); MB / OB make their norms 1.  Anchors use the rest.  A unit q
# cannot have 64 components at 0.125 (sum of squares 1.001, at the unnorm edge), so the level tops out near 0.70.
A_DIMS, B_DIMS = np.arange(0, 32), np.arange(32, 63)
QX, QF, MB, OB = 63, 64, 65, 66
FREE = np.arange(67, DIM)
HIGH_LEVEL = 0.70


def _design_q():
    q = np.zeros(DIM)
    q[A_DIMS] = rounds_down_from(0.125)                                  # f16(q) < q: products with M understated
    q[B_DIMS] = rounds_up_to(np.float16(0.125) + np.float16(2.0 ** -13))  # f16(q) > q: products with O overstated
    q[QX] = rounds_up_to(np.float16(0.118))
    return _balance(q, QF)


def _shift(row, dim, steps, down):
    """move a designed component `steps` fp16 grid points, back onto its designed side of the midpoint"""
    g = np.float16(abs(row[dim]) if row[dim] else 0)
    for _ in range(abs(steps)):
        g = np.nextafter(g, np.float16(np.inf if steps > 0 else 0))
    row[dim] = rounds_down_from(g) if down else rounds_up_to(g)


def _design_key(q, dims, level, down, bal):
    qd = q[dims].astype(np.float64)
    t = level / float(qd @ qd)
    row = np.zeros(DIM)
    for d_ in dims:
        g = np.float16(t * q[d_])
        row[d_] = rounds_down_from(g) if down else rounds_up_to(g)
    return _balance(row, bal)


def _s(q, x):
    return float(np.asarray(q, f32).astype(np.float64) @ np.asarray(x, f32).astype(np.float64))


def _m(q, x):
    return float(k_to_f16(q).astype(np.float64) @ k_to_f16(x).astype(np.float64))


def plant(k, level, rng):
    """Rows of one planted query in the designed frame (fp32, unit norm to fp32 rounding):
    {"q", "anchors" [k-1], "M", "O"}.  M at exact score ~level, understated; O overstated, its exact score just below
    M's (gap 2e-6 .. 2.5e-5).  At the high level O's screening score also sits 3 ACC .. 3 ACC + 3e-5 above a multiple of
    tau's truncation step, so the truncation takes little of the window."""
    q = _design_q()
    M = _design_key(q, A_DIMS, level, True, MB)
    O = _design_key(q, np.r_[B_DIMS, QX], level, False, OB)
    i = 0
    while _s(q, _balance(O, OB)) >= _s(q, M) - 1e-4:          # O below M
        _shift(O, B_DIMS[i % len(B_DIMS)], -1, False)
        i += 1
    if level >= HIGH_LEVEL - 0.01:
        T = 2.0 ** (np.floor(np.log2(_m(q, O))) - 23 + SEL_LOW)
        while True:
            m = _m(q, _balance(O, OB))
            if 3 * ACC <= m - np.floor(m / T) * T <= 3 * ACC + 3e-5:
                break
            _shift(O, B_DIMS[i % len(B_DIMS)], -1, False)
            i += 1
            assert i < 400
    O = _balance(O, OB)
    sO = _s(q, O)
    i = 0
    while _s(q, _balance(M, MB)) - sO > 2.5e-5:              # M: the first exact score at least 2e-6 above O's
        _shift(M, A_DIMS[i % len(A_DIMS)], -1, True)
        i += 1
    while _s(q, _balance(M, MB)) - sO < 2e-6:
        _shift(M, A_DIMS[i % len(A_DIMS)], +1, True)
        i += 1
    M = _balance(M, MB)
    # anchors: exact scores spread over [level + 0.02, level + 0.25], far above M and O in either score
    cs = np.linspace(level + 0.02, min(level + 0.25, 0.97), max(k - 1, 1))[:k - 1]
    anchors = np.zeros((k - 1, DIM))
    for j, c in enumerate(cs):
        r = np.zeros(DIM)
        r[FREE] = rng.normal(0, 1, len(FREE))
        r /= np.linalg.norm(r)
        a = c * q + np.sqrt(1 - c * c) * r
        anchors[j] = a / np.linalg.norm(a)
    return {"q": q.astype(f32), "anchors": anchors.astype(f32), "M": M.astype(f32), "O": O.astype(f32)}


def place(rows, rng):
    """a random signed permutation of the frame (error analysis unchanged: f16(-x) = -f16(x)); one per planted query
    so that two plants in one table meet at random"""
    perm = rng.permutation(DIM)
    sg = rng.choice([-1.0, 1.0], DIM)
    out = {}
    for key, x in rows.items():
        y = np.zeros_like(x)
        y[..., perm] = x * sg
        out[key] = y.astype(f32)
    out["q_free"] = int(perm[QF])      # where q's free component went
    return out


def fillers(rng, n, zero_dims=None):
    """random unit rows (fp32); with zero_dims, rows that are exactly orthogonal to a planted query"""
    X = rng.normal(0, 1, (n, DIM))
    if zero_dims is not None:
        X[:, zero_dims] = 0.0
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(f32)


def q_support(rows):
    return np.nonzero(rows["q"])[0]


def planted_table(k, level, n_plants, n_fill, seed, lead=None):
    """A key table with `n_plants` planted queries.  Key-stream order: every plant's anchors and O, then the queries,
    then the fillers, then every M — in the last key tile, where the refreshed threshold is as tight as it gets when M
    arrives.  With `lead` (the all-pairs job) the order is instead: `lead` fillers, every M, anchors and O, the other
    fillers, the queries last — so that each plant's keys lie in a later batch than the learning batch and an earlier
    one than the query's, and reach the query only through its inbox.  Below the high level the table holds one plant
    and its fillers are orthogonal to the query (random rows would outrank M).
    Returns (W fp32 [n, 128], plants: list of {"q", "M", "O", "anchors"} row indices and "q_free", the column of
    q's free component)."""
    rng = np.random.default_rng(seed)
    ps = [place(plant(k, level, rng), rng) for _ in range(n_plants)]
    zero = None
    if level < HIGH_LEVEL - 0.01:
        assert n_plants == 1
        zero = q_support(ps[0])
    fill = fillers(rng, n_fill, zero)
    blocks = [("anchors", [p["anchors"] for p in ps]), ("O", [p["O"][None] for p in ps])]
    tail = [("q", [p["q"][None] for p in ps])]
    ms = [("M", [p["M"][None] for p in ps])]
    if lead is None:
        order = blocks + tail + [("fill", [fill])] + ms
    else:
        order = [("fill", [fill[:lead]])] + ms + blocks + [("fill", [fill[lead:]])] + tail
    rows, idx, nrow = [], [dict() for _ in ps], 0
    for j, p in enumerate(ps):
        idx[j]["q_free"] = p["q_free"]
    for name, parts in order:
        for j, x in enumerate(parts):
            if name != "fill":
                idx[j][name] = list(range(nrow, nrow + len(x))) if name == "anchors" else nrow
            rows.append(x)
            nrow += len(x)
    return np.concatenate(rows).astype(f32), idx


def with_sumsq(row, target, free_dim):
    """the row with its free component (no designed component, zero in every partner) reset so that the fp64 sum of
    squares of the fp32 row is `target` (the unnorm edge)"""
    r = np.asarray(row, np.float64).copy()
    r[free_dim] = 0.0
    r[free_dim] = np.sqrt(target - np.sum(r * r)) * (1.0 if row[free_dim] >= 0 else -1.0)
    return r.astype(f32)


def subnormal_row(rng, n_small=120, small=3e-5):
    """a unit row with n_small fp16-subnormal components (|x| < 6.1e-5) beside a few dominant ones"""
    x = np.zeros(DIM)
    dims = rng.permutation(DIM)
    x[dims[:n_small]] = rng.uniform(0.2, 1.0, n_small) * small * rng.choice([-1, 1], n_small)
    big = dims[n_small:]
    x[big] = rng.normal(0, 1, len(big))
    x[big] *= np.sqrt(1 - np.sum(x[dims[:n_small]] ** 2)) / np.linalg.norm(x[big])
    return x.astype(f32)


# ---------------------------------------------------------------------------------------------------------------
# what a plant achieves under the model
# ---------------------------------------------------------------------------------------------------------------
def predict_split(W, plants):
    """model_recs form of a planted table: the queries become user rows, the other rows the anime table.
    Returns (U [n_plants, 128], A, plants with anime-table indices)."""
    qrows = np.array([d["q"] for d in plants])
    keep = np.ones(len(W), bool)
    keep[qrows] = False
    new = np.cumsum(keep) - 1
    out = [{"M": int(new[d["M"]]), "O": int(new[d["O"]]), "anchors": [int(new[a]) for a in d["anchors"]]}
           for d in plants]
    return np.asarray(W[qrows], f32), np.asarray(W[keep], f32), out


def plant_report(W, d, k, eps=EPS, exclude_self=True, qvec=None):
    """The model's view of one planted query of key table W (index dict d; model_recs form: qvec, no "q" row)."""
    Wf = np.asarray(W, f32)
    qv = Wf[d["q"]] if qvec is None else np.asarray(qvec, f32)
    s = exact(qv[None], Wf)[0]
    m = screen(k_to_f16(qv[None]), k_to_f16(Wf))[0]
    k_eff = k + int(exclude_self and qvec is None)
    tau, lo, kept = window(m, k_eff, eps)
    s_x = s.copy()
    if qvec is None and exclude_self:
        s_x[d["q"]] = -np.inf
    order = np.argsort(-s_x, kind="stable")
    rank = {int(r): i for i, r in enumerate(order[:k + 5])}
    return dict(s=s, m=m, tau=float(tau), lo=float(lo), kept=kept, order=order,
                rank_M=rank.get(d["M"]), rank_O=rank.get(d["O"]),
                err_M=(m[d["M"]] - s[d["M"]]) / EPS, err_O=(m[d["O"]] - s[d["O"]]) / EPS,
                tau_is_O=float(tau) == float(tau_trunc(m[[d["O"]]], 1)),
                margin_M=(float(f32(m[d["M"]])) - float(lo)) / EPS)
