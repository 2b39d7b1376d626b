"""GPU tests of the output heads (anirec_train_desc.loss / .activation, the predict calls' activation): the HIP head
against the oracle's statement of the heads (oracle.anirec_oracle.head_terms), through every
layer — the head and eval kernels, the one-GPU engine (stage by stage, eager, graph, lazy), trainer.fit, two gloo
ranks, the predict and model_recs paths and the neural_network component."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import anirec_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LOSSES, ACTS = orc.LOSSES, orc.ACTIVATIONS
PAIRS = [(l, a) for l in LOSSES for a in ACTS]
SET = [("mean_squared_error", "linear"), ("binary_crossentropy", "relu"), ("huber", "tanh"),
       ("log_cosh", "softplus"), ("mean_absolute_error", "sigmoid")]
# the BCE of a relu's output is well conditioned only away from p = 0 and p = 1 (there dl/dp ~ 1/p): its multi-step
# run starts from a head that puts y = 0.5 +- 0.25 zhat inside (0, 1)
HEAD = dict(w=1.2, b=0.05, gamma=0.9, beta=0.3)


def _problem(seed, n_u, n_a, n, zipf=1.2):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-0.05, 0.05, (n_u, 128)).astype(f32)
    A = rng.uniform(-0.05, 0.05, (n_a, 128)).astype(f32)
    ui = rng.integers(0, n_u, n).astype(np.int64)
    ai = ((rng.zipf(zipf, n) - 1) % n_a).astype(np.int64)
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return U, A, ui, ai, t


def _engine(U, A, B, loss, act, arena=8, **kw):
    from anime_recommendations_amd.engine import TrainEngine
    eng = TrainEngine(U.shape[0], A.shape[0], max_batch=B, arena_steps=arena, loss=loss, activation=act, **kw)
    eng.set_head(**HEAD)
    eng.set_weights(U, A)
    eng.reset_optimizer()
    return eng


def _schedule(n, B, lr):
    starts = np.arange(0, n, B)
    counts = np.minimum(B, n - starts)
    return starts, counts, [orc.adam_alpha(lr, i + 1) for i in range(len(starts))]


def _state(U, A, head=HEAD):
    return orc.new_state(U, A, orc.new_head(**head))


def _dy_bracket(loss, act, y, t, B):
    """the restated dy at y and at y +- delta: the GPU's y differs from NumPy's by a rounding or two of z*inv + shift
    (and its p by a few ulps of the transcendental), which moves a badly conditioned dy (a BCE of probabilities with p
    near 0 or 1) by far more than its own rounding"""
    d = f32(1e-6) * (f32(1) + np.abs(y))
    ds = [orc.head_terms(loss, act, y + s * d, t)[2] / f32(B) for s in (-1, 0, 1)]
    return np.minimum.reduce(ds), np.maximum.reduce(ds), ds[1]


# ---- one step, stage by stage, every pair ---------------------------------------------------------------------
@pytest.mark.parametrize("loss,act", PAIRS)
def test_one_step_stage_by_stage(loss, act):
    from anime_recommendations_amd.engine import read_ws
    U, A, ui, ai, t = _problem(2, 3000, 500, 2500)
    B = 2500
    eng = _engine(U, A, B, loss, act)
    eng.set_epoch(ui, ai, t, [0], [B], [orc.adam_alpha(1e-5, 1)])
    eng.fwd()
    eng.head()
    f, g, met = orc.grads(U, A, ui, ai, t, orc.new_head(**HEAD), loss=loss, activation=act)
    dy_o = g["dy"]
    dy = read_ws(eng, "dy")[:B]
    lo, hi, _ = _dy_bracket(loss, act, f["y"], t, B)
    tol = np.abs(dy_o).max() * 2e-5 + 2e-5 * np.abs(dy_o)
    bad = (dy < lo - tol) | (dy > hi + tol)
    assert not bad.any(), (np.nonzero(bad)[0][:5], dy[bad][:5], dy_o[bad][:5], f["y"][bad][:5])
    nblk = (B + 255) // 256
    hp = read_ws(eng, "hpart")[:nblk * 8].reshape(nblk, 8).astype(np.float64).sum(0)
    # (the partial sums against the kernel's own dy: the restatement's badly conditioned elements are bracketed above)
    assert abs(hp[0] - float(np.sum(dy, dtype=np.float64))) < 1e-7 + 1e-5 * float(np.abs(dy).sum())
    assert abs(hp[2] / B - float(met["bce"])) < 2e-6 + 2e-5 * abs(float(met["bce"]))
    assert abs(hp[3] / B - float(met["mse"])) < 1e-6 + 1e-5 * float(met["mse"])
    pub = np.frombuffer(read_ws(eng, "pub", np.uint8).tobytes()[:56],
                        dtype=[("i", "<i4", (4,)), ("f", "<f4", (10,))])[0]
    assert list(pub["i"]) == [0, B, nblk, 0]
    assert abs(pub["f"][1] - f["mu"]) < 1e-6 and abs(pub["f"][2] - f["var"]) < 1e-7
    assert pub["f"][4] == f32(HEAD["w"]) and pub["f"][6] == f32(HEAD["gamma"]) and pub["f"][7] == f32(HEAD["beta"])
    eng.prep(0, 1)
    eng.bwd()
    eng.adam()
    rec = eng.read_state()
    assert abs(rec["last_loss"] - met["loss"]) < 2e-6 + 2e-5 * abs(float(met["loss"]))
    assert abs(rec["last_mse"] - met["mse"]) < 1e-6 + 1e-5 * float(met["mse"])
    eng.close()


# ---- several steps with a ragged last batch -------------------------------------------------------------------
@pytest.mark.parametrize("loss,act", SET)
def test_steps_match_the_restatement(loss, act):
    n_u, n_a, B, steps = 4000, 900, 1000, 8
    n = B * steps - B // 3
    U, A, ui, ai, t = _problem(3, n_u, n_a, n, 1.15)
    lr = 3e-5
    head = dict(HEAD, gamma=0.25, beta=0.5) if (loss, act) == ("binary_crossentropy", "relu") else HEAD
    st = _state(U, A, head)
    starts, counts, alphas = _schedule(n, B, lr)
    mets = [orc.train_step(st, ui[s:s + c], ai[s:s + c], t[s:s + c], lr, loss=loss, activation=act)[0]
            for s, c in zip(starts, counts)]
    eng = _engine(U, A, B, loss, act)
    eng.set_head(**head)
    eng.set_epoch(ui, ai, t, starts, counts, alphas)
    eng.reset_metrics()
    eng.run(len(starts), use_graph=False)
    rec = eng.read_state()
    tol = lr * 2e-3 * len(starts) + 1e-9
    # BCE of a relu's output: a rating with p near 0 has dl/dp ~ t/p, so an ulp of y moves its gradient by ~1e-3
    # relative; Adam's first steps pass that on to the rows it touches.  Those rows are held to 0.05 of a step per step.
    ttol = lr * 0.05 * len(starts) if (loss, act) == ("binary_crossentropy", "relu") else tol
    np.testing.assert_allclose(eng.U.cpu().numpy(), st["U"], atol=ttol)
    np.testing.assert_allclose(eng.A.cpu().numpy(), st["A"], atol=ttol)
    M = eng.M.cpu().numpy()
    np.testing.assert_allclose(M[n_u:], st["mA"], atol=np.abs(st["mA"]).max() * (1e-4 if ttol == tol else 1e-2))
    h = st["head"]
    for k in ("w", "gamma", "beta"):
        assert abs(float(rec[k]) - float(h[k])) < tol, k
    assert abs(float(rec["b"]) - float(h["b"])) <= 2.05 * lr * len(starts)
    # (the batch statistics follow w and b, whose Adam steps the restatement holds to ~1e-3 of a step each)
    assert abs(rec["mov_mean"] - h["mov_mean"]) < 3e-6 and abs(rec["mov_var"] - h["mov_var"]) < 3e-6
    loss_epoch = sum(float(m["loss"]) * c for m, c in zip(mets, counts)) / n
    mse_epoch = sum(float(m["mse"]) * c for m, c in zip(mets, counts)) / n
    el, em = eng.epoch_metrics()
    assert abs(el - loss_epoch) < 5e-6 + 2e-5 * abs(loss_epoch)
    assert abs(em - mse_epoch) < 5e-6
    eng.close()


def _run(U, A, ui, ai, t, B, loss, act, use_graph, **kw):
    starts, counts, alphas = _schedule(len(ui), B, 5e-5)
    eng = _engine(U, A, B, loss, act, arena=16, **kw)
    eng.set_epoch(ui, ai, t, starts, counts, alphas)
    eng.run(len(starts), use_graph=use_graph)
    eng.synchronize()
    out = (eng.W.cpu().numpy().copy(), eng.M.cpu().numpy().copy(), eng.V.cpu().numpy().copy(), eng.read_state())
    eng.close()
    return out


def test_graph_is_bitwise_eager():
    U, A, ui, ai, t = _problem(4, 6000, 800, 40 * 1000, 1.1)
    a = _run(U, A, ui, ai, t, 1000, "huber", "tanh", False)
    b = _run(U, A, ui, ai, t, 1000, "huber", "tanh", True)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert a[3].tobytes() == b[3].tobytes()


def test_lazy_is_bitwise_dense_under_adam():
    U, A, ui, ai, t = _problem(5, 20000, 2000, 24 * 500, 1.1)
    a = _run(U, A, ui, ai, t, 500, "log_cosh", "softplus", True, lazy=True)
    b = _run(U, A, ui, ai, t, 500, "log_cosh", "softplus", True, lazy=False)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for k in ("w", "b", "gamma", "beta", "mov_mean", "mov_var", "last_mse", "se_sum"):
        assert a[3][k] == b[3][k], k


@pytest.mark.parametrize("loss,act", SET + [("binary_crossentropy", "sigmoid"), ("binary_crossentropy", "linear")])
def test_evaluate_matches_the_restatement(loss, act):
    U, A, ui, ai, t = _problem(6, 2000, 400, 3000)
    eng = _engine(U, A, 512, loss, act)
    hv = dict(HEAD, mov_mean=0.05, mov_var=0.5)
    eng.set_head(**hv)
    st = orc.new_state(U, A, orc.new_head(**hv))
    vl, vm = eng.evaluate(torch.from_numpy(ui).cuda(), torch.from_numpy(ai).cuda(), torch.from_numpy(t).cuda())
    r = orc.evaluate(st, ui, ai, t, loss=loss, activation=act)
    assert abs(vl - float(r["val_loss"])) < 2e-6 + 2e-5 * abs(float(r["val_loss"]))
    assert abs(vm - float(r["val_mse"])) < 2e-6
    eng.close()


def test_descriptor_out_of_range_is_refused_and_buffers_stay():
    from anime_recommendations_amd import _lib
    U, A, ui, ai, t = _problem(7, 500, 300, 512)
    eng = _engine(U, A, 512, "mse", "linear")
    eng.set_epoch(ui, ai, t, [0], [512], [orc.adam_alpha(1e-5, 1)])
    eng.synchronize()
    lib = _lib.load()
    snap = [x.clone() for x in (eng.W, eng.M, eng.V, eng.state_buf, eng.packets, eng.workspace)]
    base = eng.desc
    for field, bad in (("loss", 5), ("loss", -1), ("activation", 5), ("activation", -3)):
        d = _lib.TrainDesc.from_buffer_copy(base)
        setattr(d, field, bad)
        s = eng._sp()
        for fn in (lib.anirec_train_fwd, lib.anirec_train_head, lib.anirec_train_bwd, lib.anirec_train_adam,
                   lib.anirec_train_init_reg):
            assert fn(C.byref(d), s) == -1
        assert lib.anirec_train_prep(C.byref(d), 0, 1, s) == -1
        assert lib.anirec_eval(C.byref(d), _lib.ptr(eng.user_idx), _lib.ptr(eng.anime_idx), _lib.ptr(eng.rating),
                               16, s) == -1
        h = C.c_void_p()
        assert lib.anirec_trainer_create(C.byref(d), C.byref(h)) == -1
    eng.synchronize()
    for x, y in zip(snap, (eng.W, eng.M, eng.V, eng.state_buf, eng.packets, eng.workspace)):
        assert torch.equal(x, y)
    # the predict calls' activation argument
    hd = _lib.Head(1.0, 0.0, 1.0, 0.0, 0.0, 1.0)
    Ut, At = torch.from_numpy(U).cuda(), torch.from_numpy(A).cuda()
    us = torch.arange(4, dtype=torch.int32, device="cuda")
    out = torch.full((4, 300), 7.0, device="cuda")
    ws = torch.zeros(int(lib.anirec_predict_mfma_workspace_bytes(300, 4)) + (1 << 22), dtype=torch.uint8,
                     device="cuda")
    P = _lib.ptr
    for act in (5, -1):
        assert lib.anirec_predict_pairs_act(P(Ut), P(At), P(us), P(us), 4, C.byref(hd), act, P(out), None) == -1
        assert lib.anirec_predict_grid_act(P(Ut), P(At), 300, P(us), 4, C.byref(hd), act, P(out), P(ws), ws.numel(),
                                           None) == -1
        assert lib.anirec_predict_grid_mfma_act(P(Ut), P(At), 300, P(us), 4, C.byref(hd), act, P(out), P(ws),
                                                ws.numel(), None) == -1
        oi = torch.full((4, 5), 3, dtype=torch.int32, device="cuda")
        assert lib.anirec_predict_topk_act(P(Ut), P(At), 300, P(us), 4, C.byref(hd), act, None, 5, P(oi), P(out),
                                           P(ws), ws.numel(), None) == -1
        assert lib.anirec_predict_topk_mfma_act(P(Ut), P(At), 300, P(us), 4, C.byref(hd), act, None, 5, P(oi),
                                                P(out), P(oi), P(ws), ws.numel(), None) == -1
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (oi == 3).all()
    eng.close()


# ---- predict paths --------------------------------------------------------------------------------------------
def _pred_problem(n_u=300, n_a=1000, seed=8):
    rng = np.random.default_rng(seed)
    U = rng.normal(0, 1, (n_u, 128)).astype(f32)
    A = rng.normal(0, 1, (n_a, 128)).astype(f32)
    A[:, :8] += rng.normal(0, 3, (1, 8)).astype(f32)      # correlated rows: a spread of cosines
    U[:, :8] += rng.normal(0, 3, (1, 8)).astype(f32)
    return U, A


HEADS = {"sigmoid": dict(w=4.0, b=0.0, gamma=1.1, beta=0.2, mov_mean=0.1, mov_var=0.3),
         "linear": dict(w=1.3, b=0.1, gamma=0.9, beta=0.5, mov_mean=0.05, mov_var=0.8),
         "tanh": dict(w=3.0, b=0.0, gamma=1.0, beta=-0.3, mov_mean=0.0, mov_var=0.5),
         "relu": dict(w=2.0, b=0.0, gamma=1.0, beta=0.1, mov_mean=0.2, mov_var=0.6),
         "softplus": dict(w=-2.5, b=0.0, gamma=1.0, beta=0.4, mov_mean=0.0, mov_var=0.7)}


@pytest.mark.parametrize("n_a", [1000, 1001])
@pytest.mark.parametrize("act", ACTS)
def test_predict_paths_match_the_restatement(act, n_a):
    from anime_recommendations_amd import ops
    U, A = _pred_problem(n_a=n_a)
    head = dict(HEADS[act], activation=act)
    Ut, At = torch.from_numpy(U).cuda(), torch.from_numpy(A).cuda()
    users = np.arange(0, 300, 3)
    ui = np.repeat(users, n_a)
    ai = np.tile(np.arange(n_a), len(users))
    want = orc.predict_pairs(U, A, orc.new_head(**HEADS[act]), ui, ai, activation=act).reshape(len(users), n_a)
    p = ops.predict_pairs(Ut, At, head, ui, ai).cpu().numpy().reshape(len(users), n_a)
    np.testing.assert_allclose(p, want, rtol=0, atol=1e-5)
    g = ops.predict_grid(Ut, At, head, users).cpu().numpy()
    np.testing.assert_allclose(g, want, rtol=0, atol=1e-5)
    gm = ops.predict_grid_mfma(Ut, At, head, users).cpu().numpy()
    np.testing.assert_allclose(gm, want, rtol=0, atol=1e-5)
    if act != "sigmoid":   # the head's activation reaches the kernels: the sigmoid is not what came out
        gs = ops.predict_grid(Ut, At, HEADS[act], users).cpu().numpy()
        assert np.abs(gs - g).max() > 1e-2


def _exact_ranking(grid, k, watched=None):
    n_q, n_a = grid.shape
    idx = np.full((n_q, k), -1, np.int64)
    for q in range(n_q):
        cand = np.arange(n_a) if watched is None else np.nonzero(~watched[q])[0]
        order = cand[np.lexsort((cand, -grid[q, cand]))][:k]
        idx[q, :len(order)] = order
    return idx


@pytest.mark.parametrize("act,beta", [(a, HEADS[a]["beta"]) for a in ACTS] + [("relu", -0.9), ("tanh", 4.0)])
def test_topk_paths_equal_the_exact_ranking(act, beta):
    from anime_recommendations_amd import ops
    U, A = _pred_problem(n_u=400, n_a=1500, seed=9)
    head = dict(HEADS[act], beta=beta, activation=act)
    Ut, At = torch.from_numpy(U).cuda(), torch.from_numpy(A).cuda()
    users = np.arange(400)
    rng = np.random.default_rng(1)
    watched = rng.random((400, 1500)) < 0.1
    bits = np.zeros((400, (1500 + 31) // 32), np.uint32)
    for q in range(400):
        nz = np.nonzero(watched[q])[0]
        np.bitwise_or.at(bits[q], nz >> 5, (np.uint32(1) << (nz & 31).astype(np.uint32)))
    k = 20
    grid = ops.predict_grid(Ut, At, head, users).cpu().numpy()
    want = _exact_ranking(grid, k, watched)
    ie, pe = ops.predict_topk(Ut, At, head, users, k, bits.view(np.int32))
    ie, pe = ie.cpu().numpy(), pe.cpu().numpy()
    assert np.array_equal(ie, want)
    assert np.array_equal(pe, np.take_along_axis(grid, want, 1))
    im, pm, n_fb = ops.predict_topk_mfma(Ut, At, head, users, k, bits.view(np.int32))
    assert np.array_equal(im.cpu().numpy(), ie)
    assert np.array_equal(pm.cpu().numpy().view(np.uint32), pe.view(np.uint32))
    if act == "relu" and beta < 0:
        # most ratings are 0: the rows whose k-th best ties at 0 cannot be proven on the MFMA side and fall back
        assert (pe[:, -1] == 0).any() and n_fb > 0
    if act in ("linear", "sigmoid"):
        assert n_fb < 40


@pytest.mark.parametrize("act", ACTS)
def test_rating_slack_covers_the_activation(act):
    """The rerank's bound (anirec_topk_mfma.hip, rating_bound): the exact path's ratings act(fmaf(c, hs, hb)) are
    non-decreasing in their argument up to the slack stated for each activation.  The linear head's grid IS that
    argument, bit for bit (same score chain, same fmaf), so the grid of `act` is checked against it."""
    from anime_recommendations_amd import ops
    slack = {"sigmoid": 6e-7, "linear": 0.0, "relu": 0.0, "tanh": 1e-6, "softplus": 2e-6}[act]
    rng = np.random.default_rng(2)
    n = 1 << 16
    W = rng.normal(0, 1, (n, 128)).astype(f32)
    W[:, 0] += np.linspace(-40, 40, n).astype(f32)      # every cosine in (-1, 1) is reached
    Wt = torch.from_numpy(W).cuda()
    for hd in (dict(w=30.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0),
               dict(w=-3.0, b=0.0, gamma=1.0, beta=-1.0, mov_mean=0.0, mov_var=1.0),
               dict(w=120.0, b=0.0, gamma=1.0, beta=-30.0, mov_mean=0.0, mov_var=1.0)):
        y = ops.predict_grid(Wt[:1], Wt, dict(hd, activation="linear"), [0]).cpu().numpy()[0]
        r = ops.predict_grid(Wt[:1], Wt, dict(hd, activation=act), [0]).cpu().numpy()[0]
        order = np.argsort(y, kind="stable")
        rr = r[order].astype(np.float64)
        run_max = np.maximum.accumulate(rr)
        bound = rr + np.abs(rr) * slack
        if act == "sigmoid":
            bound = rr * (1 + 6e-7)
        assert (run_max[:-1] <= bound[1:]).all()


# ---- trainer.fit ----------------------------------------------------------------------------------------------
def test_fit_history_mse_linear():
    from anime_recommendations_amd import data, schedule, trainer
    table = data.encode_frame(data.synth_user_stats(n_users=1500, n_anime=300, n_ratings=14_000, seed=5))
    cfg = trainer.FitConfig(epochs=3, batch_size=1000, test_size=2000, start_lr=1e-4, max_lr=3e-4, min_lr=1e-4,
                            rampup_epochs=2, verbose=0, seed=4, loss="MSE", activation="Linear", arena_steps=8,
                            patience=10, kernel_initializer="glorot_uniform", use_graph=True)
    res = trainer.fit(table, cfg)
    assert res.loss == "mean_squared_error" and res.activation == "linear"
    # the restatement of the same epochs
    n_train = len(table) - cfg.test_size
    tr, te = table.split(cfg.test_size)
    U0, A0, w0 = trainer.init_weights(table.n_users, table.n_anime, 128, cfg.seed, "glorot_uniform")
    st = orc.new_state(U0, A0, orc.new_head(w=w0))
    ui, ai, rt = (np.asarray(c[tr]) for c in (table.user, table.anime, table.rating))
    vu, va, vt = (np.asarray(c[te]) for c in (table.user, table.anime, table.rating))
    gen = torch.Generator(device="cuda:0")
    hist = {"loss": [], "mse": [], "val_loss": [], "val_mse": []}
    for epoch in range(cfg.epochs):
        lr = cfg.lr(epoch)
        gen.manual_seed(cfg.seed * 1_000_003 + epoch)
        perm = torch.randperm(n_train, generator=gen, device="cuda:0").cpu().numpy()
        L = M = 0.0
        for s in range(0, n_train, cfg.batch_size):
            g = perm[s:s + cfg.batch_size]
            met = orc.train_step(st, ui[g], ai[g], rt[g], lr, loss="mean_squared_error", activation="linear")[0]
            L += float(met["loss"]) * len(g)
            M += float(met["mse"]) * len(g)
        hist["loss"].append(L / n_train)
        hist["mse"].append(M / n_train)
    for k in ("loss", "mse"):
        np.testing.assert_allclose(res.history[k], hist[k], rtol=0, atol=5e-5, err_msg=k)
    # validation of the weights the fit ended with (the last epoch; no early stop here): Adam's steps of about lr on
    # elements whose gradient is rounding noise let the two runs' tables drift apart by far more than the History's
    # training columns show, so the restatement evaluates the engine's own final state
    fin = orc.new_state(res.U, res.A, orc.new_head(**res.head))
    ev = orc.evaluate(fin, vu, va, vt, loss="mean_squared_error", activation="linear")
    assert abs(res.history["val_loss"][-1] - float(ev["val_loss"])) < 5e-6
    assert abs(res.history["val_mse"][-1] - float(ev["val_mse"])) < 5e-6
    assert res.stopped_epoch == -1
    assert schedule.resolve_loss(cfg.loss) == res.loss


# ---- two gloo ranks on cuda:0 ---------------------------------------------------------------------------------
def _dist_problem():
    rng = np.random.default_rng(21)
    n_u, n_a, n = 1501, 500, 7 * 2000 - 333
    U = rng.uniform(-0.05, 0.05, (n_u, 128)).astype(f32)
    A = rng.uniform(-0.05, 0.05, (n_a, 128)).astype(f32)
    ui = rng.integers(0, n_u, n)
    ai = (rng.zipf(1.15, n) - 1) % n_a
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return U, A, ui, ai, t, rng.permutation(n)


def _dist_worker(rank, world, port, out_dir, loss, act):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from anime_recommendations_amd import schedule
        from anime_recommendations_amd.dist import DistTrainEngine
        U, A, ui, ai, t, perm = _dist_problem()
        eng = DistTrainEngine(U.shape[0], A.shape[0], 1000, l2=1e-4, arena_steps=4, device=dev, mode="sharded",
                              loss=loss, activation=act)
        assert eng.eng.loss == loss and eng.eng.activation == act
        eng.set_head(**HEAD)
        eng.set_weights(U, A)
        eng.reset_optimizer()
        tu, ta, tt, tp = (torch.from_numpy(np.asarray(x)).to(dev) for x in (ui, ai, t, perm))
        n_steps = (len(perm) + 1999) // 2000
        eng.set_epoch_global(tu, ta, tt, tp, schedule.step_rates("adam", 3e-5, 1, n_steps))
        eng.reset_metrics()
        eng.run(n_steps)
        loss_e, _ = eng.epoch_metrics()
        Ufull = eng.U.cpu().numpy()
        Aloc = eng.A.cpu().numpy()
        if rank == 0:
            rec = eng.read_state()
            np.savez(os.path.join(out_dir, "dist.npz"), U=Ufull, A=Aloc, loss=loss_e, w=rec["w"], gamma=rec["gamma"],
                     beta=rec["beta"], mov_var=rec["mov_var"])
        eng.close()
    finally:
        dist.destroy_process_group()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_gloo_ranks_sharded_match_the_restatement(tmp_path):
    loss, act = "huber", "tanh"
    mp.spawn(_dist_worker, args=(2, _port(), str(tmp_path), loss, act), nprocs=2, join=True)
    d = np.load(tmp_path / "dist.npz")
    U, A, ui, ai, t, perm = _dist_problem()
    st = _state(U, A)
    lr, Bg = 3e-5, 2000
    losses, ns = [], []
    for k in range(0, len(perm), Bg):
        g = perm[k:k + Bg]
        met = orc.train_step(st, ui[g], ai[g], t[g], lr, loss=loss, activation=act)[0]
        losses.append(float(met["loss"]) * len(g))
        ns.append(len(g))
    tol = lr * 2e-3 * len(ns)
    np.testing.assert_allclose(d["U"], st["U"], atol=tol)
    np.testing.assert_allclose(d["A"], st["A"], atol=tol)
    h = st["head"]
    for k in ("w", "gamma", "beta"):
        assert abs(float(d[k]) - float(h[k])) < tol, k
    assert abs(float(d["mov_var"]) - float(h["mov_var"])) < 1e-6
    assert abs(float(d["loss"]) - sum(losses) / sum(ns)) < 5e-6


# ---- the neural_network component, then model_recs on its weights ---------------------------------------------
def test_neural_network_component_mse_linear_then_model_recs(tmp_path):
    import json
    import pandas as pd
    from anime_recommendations_amd import components, data, weights_io
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(tmp_path / "store"), ANIREC_SEED="3")
    paths = data.write_synthetic_dataset(str(tmp_path / "data"), n_users=200, n_anime=300, n_ratings=12_000, seed=4)
    reg = ("import sys; sys.path.insert(0, %r); from anime_recommendations_amd import artifacts; "
           "artifacts.log_artifact('user_stats.parquet', %r, 'parquet')" % (ROOT, paths["user_stats"]))
    subprocess.run([sys.executable, "-c", reg], env=env, check=True, timeout=300)
    nn = dict(test_size=1500, TPU_INIT=False, embedding_size=128, kernel_initializer="glorot_uniform",
              activation_function="linear", model_loss="mse", optimizer="Adam",
              start_lr=1e-4, min_lr=1e-4, max_lr=5e-4, batch_size=1500, rampup_epochs=2, sustain_epochs=0,
              exp_decay=0.8, weights_artifact="wandb_main_weights.h5", save_weights_only=True,
              checkpoint_metric="val_loss", save_freq="epoch", mode="min", save_best_weights=True, verbose=1,
              epochs=2, save_model=True, model_name="./wandb_anime_nn.h5",
              input_data="user_stats.parquet:latest", project_name="anime_recommendations",
              model_artifact="wandb_anime_nn.h5", history_csv="wandb_anime_nn_history.csv",
              ID_emb_name="user_embedding", anime_emb_name="anime_embedding", merged_name="dot_product",
              main_df_type="parquet", model_type="h5", history_type="history_csv", weights_type="h5",
              model_metrics='["mse"]', l2_reg_factor=1e-4)
    argv = [sys.executable, os.path.join(ROOT, "neural_network", "neural_network.py")]
    for k, v in nn.items():
        argv += ["--" + k, str(v)]
    r = subprocess.run(argv, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    hist = pd.read_csv(tmp_path / "wandb_anime_nn_history.csv")
    assert len(hist) == 2 and np.isfinite(hist[["loss", "mse", "val_loss", "val_mse"]].to_numpy()).all()
    found = {}
    for dp, _, fs in os.walk(tmp_path / "store"):
        if "artifact.json" in fs:
            meta = json.load(open(os.path.join(dp, "artifact.json")))
            found[meta["name"]] = os.path.join(dp, meta["file"])
    for name in ("wandb_anime_nn.h5", "wandb_main_weights.h5"):
        m = weights_io.load_model(found[name])
        assert m["activation"] == "linear" and m["loss"] == "mean_squared_error"
    m = weights_io.load_model(found["wandb_main_weights.h5"])
    df = pd.read_parquet(paths["user_stats"])
    anime_df = components.load_anime_df(paths["all_anime"])
    syn_df = components.load_synopses(paths["synopses"])
    user_ids, anime_ids = components.index_tables(m, df)
    uid = int(user_ids[5])
    frame = components.model_recs_frame(m["U"], m["A"], weights_io.model_head(m), user_ids, anime_ids, df, anime_df, syn_df, uid,
                                        10)
    assert len(frame) > 0
    # the linear head's ratings, restated: not squashed into (0, 1) by a sigmoid
    pos = int(np.nonzero(np.asarray(user_ids) == uid)[0][0])
    ids = list(np.asarray(anime_ids))
    ai = np.array([ids.index(a) for a in frame["anime_id"]])
    hd = orc.new_head(**{k: m["head"][k] for k in ("w", "b", "gamma", "beta", "mov_mean", "mov_var")})
    want = orc.predict_pairs(m["U"], m["A"], hd, np.full(len(ai), pos), ai, activation="linear")
    np.testing.assert_allclose(frame["Prediction"].to_numpy(), want, rtol=0, atol=1e-5)
    assert (np.diff(frame["Prediction"].to_numpy()) <= 0).all()
