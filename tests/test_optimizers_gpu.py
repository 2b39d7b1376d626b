"""GPU tests of the SGD / RMSprop / Adagrad train step (anirec_train_desc.optimizer): the HIP update against the
oracle's statement of the Keras-2.12 rules (include/anirec.h, ANIREC_OPT_*; oracle.anirec_oracle.opt_update) on the
oracle's gradients, through every layer — the flat kernel, the one-GPU engine (graph, eager and stage by
stage), trainer.fit, two gloo ranks, the neural_network component."""
import json
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
from oracle.anirec_oracle import KINDS, SLOT_INIT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- the flat kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_opt_flat_is_bitwise_the_restatement(kind):
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(11)
    n = 1 << 20
    w = rng.normal(0, 0.05, n).astype(f32)
    w[:64] = 0.0
    w[64:128] = -0.0
    g = rng.normal(0, 1e-4, n).astype(f32)
    g[128:192] = 0.0
    g[192:256] = -0.0
    g[256:320] = rng.choice([-1, 1], 64) * f32(1e-20)          # g*g underflows
    g[320:384] = rng.choice([-1, 1], 64) * f32(1e-30)
    g[384:448] = rng.choice([-1, 1], 64) * f32(1e19)           # g*g overflows to inf: the step is a signed zero
    g[448:512] = rng.choice([-1, 1], 64) * f32(3e3)
    s = (rng.random(n) * 1e-6).astype(f32) + f32(SLOT_INIT[kind])
    s[512:576] = f32(SLOT_INIT[kind])
    lr = f32(4.2e-5)
    tw, ts, tg = (torch.from_numpy(x.copy()).cuda() for x in (w, s, g))
    ops.opt_flat(kind, tw, None if kind == "sgd" else ts, tg, lr)
    torch.cuda.synchronize()
    orc.opt_update(kind, w, None, s, g, lr)
    assert np.array_equal(tw.cpu().numpy().view(np.uint32), w.view(np.uint32))
    if kind != "sgd":
        assert np.array_equal(ts.cpu().numpy().view(np.uint32), s.view(np.uint32))


def test_opt_flat_refuses_adam_and_unknown_kinds():
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    x = torch.zeros(16, dtype=torch.float32, device="cuda:0")
    p = _lib.ptr(x)
    assert lib.anirec_opt_flat(_lib.OPT_ADAM, p, p, p, 16, 1e-3, None) == -1
    assert lib.anirec_opt_flat(7, p, p, p, 16, 1e-3, None) == -1
    assert lib.anirec_opt_flat(_lib.OPT_RMSPROP, p, None, p, 16, 1e-3, None) == -1


# ---- the one-GPU engine ---------------------------------------------------------------------------------------
def _problem(seed, n_u, n_a, n, zipf=1.2):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-0.05, 0.05, (n_u, 128)).astype(f32)
    A = rng.uniform(-0.05, 0.05, (n_a, 128)).astype(f32)
    ui = rng.integers(0, n_u, n).astype(np.int64)
    ai = ((rng.zipf(zipf, n) - 1) % n_a).astype(np.int64)
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return U, A, ui, ai, t


def _engine(kind, U, A, B, arena=8, **kw):
    from anime_recommendations_amd.engine import TrainEngine
    eng = TrainEngine(U.shape[0], A.shape[0], max_batch=B, arena_steps=arena, optimizer=kind, **kw)
    eng.set_head(w=1.2)
    eng.set_weights(U, A)
    eng.reset_optimizer()
    return eng


def _epoch(kind, eng, ui, ai, t, B, lr):
    from anime_recommendations_amd import schedule
    n = len(ui)
    starts = np.arange(0, n, B)
    counts = np.minimum(B, n - starts)
    eng.set_epoch(ui, ai, t, starts, counts, schedule.step_rates(kind, lr, 1, len(starts)))
    return starts, counts


def _snapshot(eng):
    eng.synchronize()
    return eng.W.cpu().numpy().copy(), eng.V.cpu().numpy().copy(), eng.M.cpu().numpy().copy(), eng.read_state()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_u,n_a,B,steps,zipf", [(300, 200, 256, 1, 1.3), (4000, 900, 1000, 10, 1.15)])
def test_engine_run_matches_the_restated_update(kind, n_u, n_a, B, steps, zipf):
    n = B * steps - (B // 3 if steps > 1 else 0)      # ragged last batch
    U, A, ui, ai, t = _problem(3, n_u, n_a, n, zipf)
    lr = 3e-5
    st = orc.new_state(U, A, orc.new_head(w=1.2), optimizer=kind)
    eng = _engine(kind, U, A, B)
    starts, counts = _epoch(kind, eng, ui, ai, t, B, lr)
    mets = [orc.train_step(st, ui[s:s + c], ai[s:s + c], t[s:s + c], lr)[0] for s, c in zip(starts, counts)]
    eng.run(len(starts), use_graph=False)
    rec = eng.read_state()
    assert rec["step_fwd"] == len(starts)
    # the oracle test's bars (test_train_gpu.test_train_steps_match_oracle)
    tol = lr * 2e-3 * len(starts) + 1e-9
    np.testing.assert_allclose(eng.U.cpu().numpy(), st["U"], atol=tol)
    np.testing.assert_allclose(eng.A.cpu().numpy(), st["A"], atol=tol)
    V = eng.V.cpu().numpy()
    if kind != "sgd":
        for got, want in ((V[:n_u], st["vU"]), (V[n_u:], st["vA"])):
            np.testing.assert_allclose(got, want, atol=np.abs(want).max() * 1e-4)
        np.testing.assert_allclose(np.array(rec["adam_v"]), st["head"]["v"], atol=np.abs(st["head"]["v"]).max() * 1e-4)
    else:
        assert (V == 0).all() and (np.array(rec["adam_v"]) == 0).all()
    assert (eng.M.cpu().numpy() == 0).all() and (np.array(rec["adam_m"]) == 0).all()   # Adam's m is never touched
    h = st["head"]
    for k in ("w", "gamma", "beta"):
        assert abs(float(rec[k]) - float(h[k])) < tol, k
    assert abs(float(rec["b"]) - float(h["b"])) <= 2.05 * lr * len(starts)
    assert abs(rec["mov_mean"] - h["mov_mean"]) < 1e-6 and abs(rec["mov_var"] - h["mov_var"]) < 1e-6
    assert abs(rec["last_loss"] - mets[-1]["loss"]) < 5e-6
    loss_epoch = sum(float(m["loss"]) * c for m, c in zip(mets, counts)) / n
    assert abs(eng.epoch_metrics()[0] - loss_epoch) < 5e-6
    assert (eng.rowmap.cpu().numpy() == 0).all()
    eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_graph_eager_and_stage_by_stage_are_bitwise_equal(kind):
    U, A, ui, ai, t = _problem(4, 3000, 600, 13 * 700 - 211, 1.1)
    B, lr = 700, 5e-5
    outs = []
    for how in ("eager", "graph", "stages"):
        eng = _engine(kind, U, A, B, arena=8)
        starts, _ = _epoch(kind, eng, ui, ai, t, B, lr)
        if how == "stages":
            for i in range(len(starts)):
                eng.prep(i, 1)
                eng.fwd(); eng.head(); eng.bwd(); eng.adam()
        else:
            eng.run(len(starts), use_graph=how == "graph")
        outs.append(_snapshot(eng))
        eng.close()
    W0, V0, M0, r0 = outs[0]
    assert np.isfinite(W0).all() and not np.array_equal(W0[:3000], U)
    for W, V, M, rec in outs[1:]:
        assert np.array_equal(W.view(np.uint32), W0.view(np.uint32)) and np.array_equal(V.view(np.uint32), V0.view(np.uint32))
        assert np.array_equal(M, M0)
        assert rec.tobytes() == r0.tobytes()


def test_adagrad_starts_from_its_initial_accumulator():
    U, A, ui, ai, t = _problem(5, 500, 300, 400, 1.3)
    lr = 4e-5
    from anime_recommendations_amd.engine import TrainEngine
    eng = TrainEngine(500, 300, max_batch=400, arena_steps=4, optimizer="Adagrad")   # fresh: no reset_optimizer call
    eng.set_weights(U, A)
    assert (eng.V.cpu().numpy() == f32(0.1)).all() and (eng.M.cpu().numpy() == 0).all()
    assert (np.array(eng.read_state()["adam_v"]) == f32(0.1)).all()
    eng.set_head(w=1.2)
    assert (np.array(eng.read_state()["adam_v"]) == f32(0.1)).all()
    st = orc.new_state(U, A, orc.new_head(w=1.2), optimizer="adagrad")
    _epoch("adagrad", eng, ui, ai, t, 400, lr)
    orc.train_step(st, ui, ai, t, lr)
    eng.run(1, use_graph=False)
    rec = eng.read_state()
    np.testing.assert_allclose(eng.U.cpu().numpy(), st["U"], atol=lr * 2e-3 + 1e-9)
    np.testing.assert_allclose(eng.A.cpu().numpy(), st["A"], atol=lr * 2e-3 + 1e-9)
    V = eng.V.cpu().numpy()
    np.testing.assert_allclose(V, np.concatenate([st["vU"], st["vA"]]), rtol=1e-6)
    for k in ("w", "gamma", "beta"):
        assert abs(float(rec[k]) - float(st["head"][k])) < lr * 2e-3 + 1e-9, k
    st2 = eng.optimizer_state(iterations=1)
    assert sorted(st2) == ["anime_embedding/accumulator", "head/accumulator", "iterations",
                           "user_embedding/accumulator"]
    eng.close()


def test_optimizer_state_keras_slot_names():
    U, A, *_ = _problem(6, 50, 40, 10)
    names = {"sgd": ["iterations"],
             "rmsprop": ["anime_embedding/velocity", "head/velocity", "iterations", "user_embedding/velocity"],
             "adam": ["anime_embedding/m", "anime_embedding/v", "head/m", "head/v", "iterations", "user_embedding/m",
                      "user_embedding/v"]}
    for kind, want in names.items():
        eng = _engine(kind, U, A, 16, arena=4)
        assert sorted(eng.optimizer_state(3)) == want
        eng.close()


def test_lazy_is_adam_only():
    from anime_recommendations_amd.engine import TrainEngine
    for kind in ("SGD", "rmsprop", "adagrad"):
        with pytest.raises(ValueError):
            TrainEngine(9000, 100, max_batch=1000, arena_steps=4, optimizer=kind, lazy=True)
    with pytest.raises(ValueError):
        TrainEngine(100, 100, max_batch=10, arena_steps=4, optimizer="nadam")
    # tables of >= 8 batches' worth of rows: Adam takes the lazy update automatically, the other kinds the dense one
    # (ANIREC_LAZY_ADAM=1 included: it only concerns Adam)
    big = dict(max_batch=1000, arena_steps=4)
    old = os.environ.get("ANIREC_LAZY_ADAM")
    try:
        for env in (None, "1"):
            if env is None:
                os.environ.pop("ANIREC_LAZY_ADAM", None)
            else:
                os.environ["ANIREC_LAZY_ADAM"] = env
            e = TrainEngine(9000, 100, **big)
            assert e.lazy
            e.close()
            for kind in KINDS:
                e = TrainEngine(9000, 100, optimizer=kind, **big)
                assert not e.lazy and e.lazy_state is None and e.desc.lazy == 0 and e.desc.optimizer > 0
                e.close()
    finally:
        if old is None:
            os.environ.pop("ANIREC_LAZY_ADAM", None)
        else:
            os.environ["ANIREC_LAZY_ADAM"] = old


def test_descriptor_with_lazy_and_another_kind_is_refused_everywhere():
    import ctypes as C
    from anime_recommendations_amd import _lib
    U, A, ui, ai, t = _problem(7, 400, 200, 300)
    eng = _engine("sgd", U, A, 300, arena=4)
    _epoch("sgd", eng, ui, ai, t, 300, 1e-5)
    lib, sp = eng.lib, eng._sp()
    for lazy, opt in ((1, _lib.OPT_SGD), (1, _lib.OPT_ADAGRAD), (0, 4), (0, -1)):
        d = _lib.TrainDesc.from_buffer_copy(eng.desc)
        d.lazy, d.optimizer = lazy, opt
        dp = C.byref(d)
        h = C.c_void_p()
        for rc in (lib.anirec_train_init_reg(dp, sp), lib.anirec_train_prep(dp, 0, 1, sp), lib.anirec_train_fwd(dp, sp),
                   lib.anirec_train_head(dp, sp), lib.anirec_train_bwd(dp, sp), lib.anirec_train_adam(dp, sp),
                   lib.anirec_train_adam_part(dp, 1, sp), lib.anirec_train_stage_ticks(dp, 0, None, None, sp),
                   lib.anirec_trainer_create(dp, C.byref(h)), lib.anirec_dist_stepper_create(dp, C.byref(h)),
                   lib.anirec_eval(dp, _lib.ptr(eng.user_idx), _lib.ptr(eng.anime_idx), _lib.ptr(eng.rating), 10, sp)):
            assert rc == -1, (lazy, opt, rc)
    eng.synchronize()
    eng.close()


# ---- trainer.fit ----------------------------------------------------------------------------------------------
def _oracle_fit(kind, table, cfg, dev):
    """trainer.fit restated on the oracle: same initial weights, same epoch shuffles (torch's generator on the
    device), History columns from the per-step metrics."""
    from anime_recommendations_amd import trainer
    tr, te = table.split(cfg.test_size)
    n_train = tr.stop - tr.start
    U0, A0, w0 = trainer.init_weights(table.n_users, table.n_anime, 128, cfg.seed)
    st = orc.new_state(U0, A0, orc.new_head(w=w0), optimizer=kind)
    ui, ai, rt = table.user[tr], table.anime[tr], table.rating[tr].astype(f32)
    vu, va, vt = table.user[te], table.anime[te], table.rating[te].astype(f32)
    gen = torch.Generator(device=dev)
    hist = {"loss": [], "mse": [], "val_loss": [], "val_mse": [], "lr": []}
    for epoch in range(cfg.epochs):
        lr = cfg.lr(epoch)
        gen.manual_seed(cfg.seed * 1_000_003 + epoch)
        perm = torch.randperm(n_train, generator=gen, device=dev).cpu().numpy()
        lw = se = 0.0
        for s in range(0, n_train, cfg.batch_size):
            p = perm[s:s + cfg.batch_size]
            met, _, _ = orc.train_step(st, ui[p], ai[p], rt[p], lr, cfg.l2_reg_factor)
            lw += float(met["loss"]) * len(p)
            se += float(met["mse"]) * len(p)
        ev = orc.evaluate(st, vu, va, vt, cfg.l2_reg_factor)
        for k, v in (("loss", lw / n_train), ("mse", se / n_train), ("val_loss", float(ev["val_loss"])),
                     ("val_mse", float(ev["val_mse"])), ("lr", float(f32(lr)))):
            hist[k].append(v)
    return hist, st


@pytest.mark.parametrize("kind", KINDS)
def test_fit_history_agrees_with_an_oracle_driven_fit(kind):
    from anime_recommendations_amd import data, trainer
    df = data.synth_user_stats(n_users=1500, n_anime=300, n_ratings=14_000, seed=5)
    table = data.encode_frame(df)
    cfg = trainer.FitConfig(epochs=3, batch_size=1000, test_size=2000, verbose=0, seed=2, arena_steps=8,
                            start_lr=1e-3, max_lr=3e-3, min_lr=1e-3, rampup_epochs=2, patience=10,
                            optimizer=kind.upper() if kind == "sgd" else kind)
    res = trainer.fit(table, cfg)
    assert res.optimizer_name == kind
    hist, st = _oracle_fit(kind, table, cfg, torch.device("cuda:0"))
    assert res.history["lr"] == hist["lr"]
    for k in ("loss", "val_loss"):
        np.testing.assert_allclose(res.history[k], hist[k], rtol=0, atol=5e-5, err_msg=k)
    for k in ("mse", "val_mse"):
        np.testing.assert_allclose(res.history[k], hist[k], rtol=0, atol=2e-5, err_msg=k)
    tol = 3e-3 * 2e-3 * 3 * 10 + 1e-9
    np.testing.assert_allclose(res.U, st["U"], atol=tol)
    np.testing.assert_allclose(res.A, st["A"], atol=tol)
    U0, A0, _ = trainer.init_weights(table.n_users, table.n_anime, 128, cfg.seed)
    assert not np.array_equal(res.A, A0)


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


def _dist_worker(rank, world, port, out_dir, mode, kind):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from anime_recommendations_amd import schedule
        from anime_recommendations_amd.dist import DistTrainEngine
        U, A, ui, ai, t, perm = _dist_problem()
        eng = DistTrainEngine(U.shape[0], A.shape[0], 1000, l2=1e-4, arena_steps=4, device=dev, mode=mode,
                              optimizer=kind)
        assert not eng.eng.lazy and eng.optimizer == kind
        eng.set_head(w=1.2)
        eng.set_weights(U, A)
        eng.reset_optimizer()
        tu, ta, tt, tp = (torch.from_numpy(np.asarray(x)).to(dev) for x in (ui, ai, t, perm))
        n_steps = (len(perm) + 1999) // 2000
        eng.set_epoch_global(tu, ta, tt, tp, schedule.step_rates(kind, 3e-5, 1, n_steps))
        eng.reset_metrics()
        eng.run(n_steps)
        loss, _ = eng.epoch_metrics()
        Ufull = eng.U.cpu().numpy()
        Aloc = eng.A.cpu().numpy()
        opt = eng.optimizer_state(iterations=n_steps)
        if rank == 0:
            rec = eng.read_state()
            slots = {k.replace("/", "__"): v for k, v in opt.items()}
            np.savez(os.path.join(out_dir, "dist.npz"), U=Ufull, A=Aloc, loss=loss, w=rec["w"], gamma=rec["gamma"],
                     beta=rec["beta"], mov_var=rec["mov_var"], **slots)
        eng.close()
    finally:
        dist.destroy_process_group()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("kind", ["sgd", "adagrad"])
@pytest.mark.parametrize("mode", ["sharded", "replicated_rs"])
def test_two_gloo_ranks_match_the_restatement(tmp_path, mode, kind):
    mp.spawn(_dist_worker, args=(2, _port(), str(tmp_path), mode, kind), nprocs=2, join=True)
    d = np.load(tmp_path / "dist.npz")
    U, A, ui, ai, t, perm = _dist_problem()
    st = orc.new_state(U, A, orc.new_head(w=1.2), optimizer=kind)
    lr, Bg = 3e-5, 2000
    losses, ns = [], []
    for k in range(0, len(perm), Bg):
        g = perm[k:k + Bg]
        met, _, _ = orc.train_step(st, ui[g], ai[g], t[g], lr)
        losses.append(float(met["loss"]) * len(g))
        ns.append(len(g))
    tol = lr * 2e-3 * len(ns)
    np.testing.assert_allclose(d["U"], st["U"], atol=tol)
    np.testing.assert_allclose(d["A"], st["A"], atol=tol)
    if kind == "adagrad":
        np.testing.assert_allclose(d["user_embedding__accumulator"], st["vU"], rtol=1e-6)
        np.testing.assert_allclose(d["anime_embedding__accumulator"], st["vA"], rtol=1e-6)
    else:
        assert "user_embedding__m" not in d.files and "iterations" in d.files
    h = st["head"]
    for k in ("w", "gamma", "beta"):
        assert abs(float(d[k]) - float(h[k])) < tol, k
    assert abs(float(d["mov_var"]) - float(h["mov_var"])) < 1e-6
    assert abs(float(d["loss"]) - sum(losses) / sum(ns)) < 5e-6


# ---- the neural_network component -----------------------------------------------------------------------------
def test_neural_network_component_trains_with_rmsprop(tmp_path):
    from anime_recommendations_amd import data, weights_io
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(tmp_path / "store"), ANIREC_SEED="3")
    paths = data.write_synthetic_dataset(str(tmp_path / "data"), n_users=200, n_anime=300, n_ratings=12_000, seed=4)
    reg = ("import sys; sys.path.insert(0, %r); from anime_recommendations_amd import artifacts; "
           "artifacts.log_artifact('user_stats.parquet', %r, 'parquet')" % (ROOT, paths["user_stats"]))
    subprocess.run([sys.executable, "-c", reg], env=env, check=True, timeout=300)
    nn = dict(test_size=1500, TPU_INIT=False, embedding_size=128, kernel_initializer="he_normal",
              activation_function="sigmoid", model_loss="binary_crossentropy", optimizer="RMSprop",
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
    import pandas as pd
    hist = pd.read_csv(tmp_path / "wandb_anime_nn_history.csv")
    assert len(hist) == 2 and np.isfinite(hist[["loss", "mse", "val_loss", "val_mse"]].to_numpy()).all()
    store = tmp_path / "store"
    found = {}
    for dp, _, fs in os.walk(store):
        if "artifact.json" in fs:
            meta = json.load(open(os.path.join(dp, "artifact.json")))
            found[meta["name"]] = (meta, os.path.join(dp, meta["file"]))
    meta, mfile = found["wandb_anime_nn.h5"]
    assert meta["metadata"]["Optimizer"] == "RMSprop"
    m = weights_io.load_model(mfile)
    assert m["optimizer_name"] == "rmsprop"
    assert sorted(m["optimizer"]) == ["anime_embedding/velocity", "head/velocity", "iterations",
                                      "user_embedding/velocity"]
    assert m["optimizer"]["user_embedding/velocity"].shape == m["U"].shape
    assert (m["optimizer"]["anime_embedding/velocity"] > 0).any()
    assert "wandb_main_weights.h5" in found
