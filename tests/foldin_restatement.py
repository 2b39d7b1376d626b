"""NumPy restatement of the fold-in of one new user (include/anirec.h, anirec_fold_in): the reference's Keras model
(neural_network.py:66-106) with every layer frozen except a fresh one-row user embedding, BatchNorm in inference
mode, model.fit full-batch on the user's ratings with Keras-2.12 Adam.  Parameterised by dtype (float32: the
kernel's operations in NumPy's summation order; float64: the yardstick of the GPU tests), loss and activation; the
per-rating head is the oracle's ``head_terms``, the statement the train step's heads are held to."""
import numpy as np

from oracle import anirec_oracle as orc

f32 = np.float32
L2N_EPS = 1e-12            # tf.nn.l2_normalize epsilon (Dot(normalize=True))
BN_EPS = 1e-3              # BatchNormalization epsilon
ADAM_EPS = 1e-7
KINK_MARGIN = 1e-4         # no rating may sit this close to a point where its gradient jumps (see kink_distance)
LOSSES = ("binary_crossentropy", "mean_squared_error", "mean_absolute_error", "huber", "log_cosh")
ACTIVATIONS = ("sigmoid", "linear", "tanh", "relu", "softplus")


def head_affine_f32(head):
    """hs, hb of y = c * hs + hb, folded in fp32 as tf.nn.batch_normalization does (head_affine_f32 of the library)"""
    w, b, gamma, beta, mu, var = (f32(head[k]) for k in ("w", "b", "gamma", "beta", "mov_mean", "mov_var"))
    inv = f32(f32(1) / np.sqrt(f32(var + f32(BN_EPS)), dtype=f32)) * gamma
    return f32(w * inv), f32(f32(b * inv) + f32(beta - f32(mu * inv)))


def normalised_rows(A, dt):
    """A with rows scaled by 1 / sqrt(max(sum a^2, 1e-12)) (the train step's forward)"""
    A = np.asarray(A, f32).astype(dt)
    ss = np.sum(A * A, axis=1, dtype=dt)
    return (A * (dt(1) / np.sqrt(np.maximum(ss, dt(L2N_EPS)), dtype=dt))[:, None]).astype(dt)


def kink_distance(loss, act, y, p, t):
    """distance of the ratings from the nearest point where dl/dy is discontinuous: y = 0 for relu, p = t for
    mean_absolute_error, |p - t| = 1 for huber, p = 1e-7 and p = 1 - 1e-7 for the clipped binary_crossentropy of a head
    other than the sigmoid's (inf for the smooth heads)"""
    d = np.inf
    y, p, t = (np.asarray(x, np.float64) for x in (y, p, t))
    if len(t) == 0:
        return d
    if act == "relu":
        d = min(d, float(np.abs(y).min()))
    if loss == "mean_absolute_error":
        d = min(d, float(np.abs(p - t).min()))
    if loss == "huber":
        d = min(d, float(np.abs(np.abs(p - t) - 1.0).min()))
    if loss == "binary_crossentropy" and act != "sigmoid":
        d = min(d, float(np.abs(p - 1e-7).min()), float(np.abs(p - (1.0 - 1e-7)).min()))
    return d


def loss_and_grad(u, Ah, t, hs, hb, l2, loss, act, dt):
    """(L, grad, kink distance) at row u: L = (1/n) sum l(p_i, t_i) + l2 sum u^2, grad = dL/du in the closed form of
    the header.  Ah: the user's normalised anime rows [n, D]."""
    n = dt(len(t))
    ss = np.sum(u * u, dtype=dt)
    ru = dt(1) / np.sqrt(np.maximum(ss, dt(L2N_EPS)), dtype=dt)
    uh = (u * ru).astype(dt)
    c = np.sum(Ah * uh[None, :], axis=1, dtype=dt)
    y = (c * dt(hs) + dt(hb)).astype(dt)
    p, li, gy = orc.head_terms(loss, act, y, t, dt)
    L = dt(np.sum(li, dtype=dt) / n + dt(l2) * ss)
    dc = ((gy / n) * dt(hs)).astype(dt)
    gsum = np.sum(dc[:, None] * (Ah - c[:, None] * uh[None, :]), axis=0, dtype=dt)
    grad = (ru * gsum + dt(2) * dt(l2) * u).astype(dt)
    return L, grad, kink_distance(loss, act, y, p, t)


def adam_update(u, m, v, g, alpha, dt):
    """Keras-2.12 Adam, in place, with the kernels' fp32 constants (float32(0.1), float32(0.001), float32(1e-7)) in
    either dtype: at float32 this is the oracle's adam_update"""
    m += (g - m) * dt(f32(0.1))
    v += (g * g - v) * dt(f32(0.001))
    u -= (m * dt(f32(alpha))) / (np.sqrt(v, dtype=dt) + dt(f32(ADAM_EPS)))


def fold_in(A, head, anime_idx, rating, init, alphas, l2=1e-4, loss="binary_crossentropy", act="sigmoid",
            dtype=np.float64, snapshots=(), check_kinks=True):
    """One user.  ``alphas``: schedule.adam_alphas(lr, 1, steps) (fp32).  Returns dict(row, loss: L at the final row,
    losses: [L_1 .. L_steps] (L_s = the loss at the row BEFORE step s), kink: the smallest kink distance met,
    snap: {s: (row after s steps, L at that row)} for s in ``snapshots``).  No ratings: the start row and a NaN loss.
    With ``check_kinks`` the run asserts that no rating ever comes within KINK_MARGIN of a gradient jump, where the
    precision of the arithmetic, not the definition, would pick the branch."""
    dt = dtype
    u = np.asarray(init, f32).astype(dt).copy()
    idx = np.asarray(anime_idx, np.int64)
    t = np.asarray(rating, f32).astype(dt)
    out = dict(losses=[], kink=np.inf, snap={})
    if len(idx) == 0:
        out.update(row=u, loss=dt("nan"))
        for s in snapshots:
            out["snap"][s] = (u.copy(), dt("nan"))
        return out
    hs, hb = head_affine_f32(head)
    Ah = normalised_rows(A, dt)[idx]
    m, v = np.zeros_like(u), np.zeros_like(u)
    steps = len(alphas)
    for s in range(steps + 1):
        L, g, kd = loss_and_grad(u, Ah, t, hs, hb, l2, loss, act, dt)
        out["kink"] = min(out["kink"], kd)
        if s in snapshots:
            out["snap"][s] = (u.copy(), L)
        if s == steps:
            break
        out["losses"].append(L)
        adam_update(u, m, v, g, alphas[s], dt)
    if check_kinks:
        assert out["kink"] > KINK_MARGIN, "a rating came within %g of a gradient jump (%s, %s)" % (out["kink"], loss, act)
    out.update(row=u, loss=L)
    return out


def fold_in_many(A, head, offsets, anime_idx, rating, init, alphas, **kw):
    """every user of a CSR; ``init``: [n_new, D].  Returns the list of the users' dicts."""
    return [fold_in(A, head, anime_idx[offsets[j]:offsets[j + 1]], rating[offsets[j]:offsets[j + 1]], init[j], alphas, **kw)
            for j in range(len(offsets) - 1)]
