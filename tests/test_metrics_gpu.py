"""GPU tests of the Keras metrics (--model_metrics): the head's metrics instantiation through anirec_trainer_run (eager,
graph, dense, lazy) and anirec_eval_metrics against tests/metrics_restatement.py, training bitwise unchanged by them,
two gloo ranks against one GPU, and the neural_network component with checkpointing on val_auc."""
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

import metrics_restatement as mr
from oracle import anirec_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
HEAD = dict(w=1.2, b=0.05, gamma=0.9, beta=0.3)
ALL = 127                     # every ANIREC_METRIC_* bit
NO_AUC = ALL & ~64


def _problem(seed, n_u, n_a, n):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-0.05, 0.05, (n_u, 128)).astype(f32)
    A = rng.uniform(-0.05, 0.05, (n_a, 128)).astype(f32)
    ui = rng.integers(0, n_u, n).astype(np.int64)
    ai = ((rng.zipf(1.15, n) - 1) % n_a).astype(np.int64)
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return U, A, ui, ai, t


def _schedule(n, B, lr):
    starts = np.arange(0, n, B)
    counts = np.minimum(B, n - starts)
    return starts, counts, [orc.adam_alpha(lr, i + 1) for i in range(len(starts))]


def _train(U, A, ui, ai, t, B, loss, act, metrics, use_graph, lazy, lr=3e-5):
    from anime_recommendations_amd.engine import TrainEngine
    eng = TrainEngine(U.shape[0], A.shape[0], max_batch=B, arena_steps=8, loss=loss, activation=act, lazy=lazy,
                      metrics=metrics)
    eng.set_head(**HEAD)
    eng.set_weights(U, A)
    eng.reset_optimizer()
    starts, counts, alphas = _schedule(len(ui), B, lr)
    eng.set_epoch(ui, ai, t, starts, counts, alphas)
    eng.reset_metrics()
    eng.run(len(starts), use_graph=use_graph)
    eng.synchronize()
    out = dict(W=eng.W.cpu().numpy().copy(), M=eng.M.cpu().numpy().copy(), V=eng.V.cpu().numpy().copy(),
               state=eng.read_state(), acc=eng.read_metric_acc("train"), logs=eng.epoch_logs())
    eng.close()
    return out


def _check_acc(acc, rec, want, mask, n):
    """GPU accumulator against the restatement: rel 1e-5 (accuracy: up to the ratings at the 0.5 threshold), AUC
    abs 1e-5 with the total bin mass exact"""
    assert rec["n_seen"] == n
    for k, kind in enumerate(mr.KINDS):
        got = float(acc["sum"][k])
        if not mask & (1 << k):
            assert got == 0.0, kind
            continue
        w = want.sum[kind]
        if kind == "accuracy":
            assert abs(got - w) <= want.near_half, (got, w)
        else:
            assert abs(got - w) <= 1e-5 * abs(w) + 1e-6, (kind, got, w)
    if mask & 64:
        tot = int(acc["auc_pos"].sum()) + int(acc["auc_neg"].sum())
        assert tot == n * mr.ONE
        assert int(acc["auc_pos"].sum()) == int(want.pos.sum())
        assert abs(mr.auc_from_bins(acc["auc_pos"], acc["auc_neg"]) - want.values()["auc"]) < 1e-5
    else:
        assert not acc["auc_pos"].any() and not acc["auc_neg"].any()


CASES = [("binary_crossentropy", "sigmoid", ALL), ("mean_squared_error", "linear", NO_AUC),
         ("log_cosh", "softplus", NO_AUC), ("huber", "tanh", NO_AUC), ("mean_absolute_error", "sigmoid", ALL),
         ("binary_crossentropy", "relu", ALL & ~64 & ~16)]


@pytest.mark.parametrize("loss,act,mask", CASES)
@pytest.mark.parametrize("use_graph,lazy", [(False, False), (True, False), (True, True)])
def test_train_metrics_match_the_restatement_and_leave_training_alone(loss, act, mask, use_graph, lazy):
    n_u, n_a, B, steps = 6000, 900, 1000, 8
    n = B * steps - 377
    U, A, ui, ai, t = _problem(11, n_u, n_a, n)
    lr = 3e-5
    on = _train(U, A, ui, ai, t, B, loss, act, mask, use_graph, lazy, lr)
    off = _train(U, A, ui, ai, t, B, loss, act, 0, use_graph, lazy, lr)
    # metrics must not perturb training: tables, moments and state bitwise
    for k in ("W", "M", "V"):
        assert np.array_equal(on[k].view(np.uint32), off[k].view(np.uint32)), k
    assert on["state"].tobytes() == off["state"].tobytes()
    st = orc.new_state(U, A, orc.new_head(**HEAD))
    starts, counts, _ = _schedule(n, B, lr)
    want = mr.train_steps(st, ui, ai, t, starts, counts, lr, loss, act)
    _check_acc(on["acc"], on["state"], want, mask, n)
    lg, wv = on["logs"], want.values()
    assert abs(lg["mse"] - wv["mse"]) < 1e-6 and abs(lg["rmse"] - wv["rmse"]) < 2e-6
    loss_e, mse_e = off_metrics = (float(off["state"]["loss_wsum"] / n), float(off["state"]["se_sum"] / n))
    assert lg["loss"] == loss_e and lg["mse"] == mse_e, off_metrics


def test_two_identical_runs_give_identical_bits():
    U, A, ui, ai, t = _problem(12, 5000, 700, 12 * 800)
    a = _train(U, A, ui, ai, t, 800, "binary_crossentropy", "sigmoid", ALL, True, True)
    b = _train(U, A, ui, ai, t, 800, "binary_crossentropy", "sigmoid", ALL, True, True)
    # integer bins: bitwise; the fp64 sums' atomics may add in another order, far below the History's fp32
    assert a["acc"]["auc_pos"].tobytes() == b["acc"]["auc_pos"].tobytes()
    assert a["acc"]["auc_neg"].tobytes() == b["acc"]["auc_neg"].tobytes()
    assert a["state"].tobytes() == b["state"].tobytes()
    for k in a["logs"]:
        assert f32(a["logs"][k]).tobytes() == f32(b["logs"][k]).tobytes(), k


@pytest.mark.parametrize("loss,act,mask", CASES)
def test_eval_metrics_match_the_restatement(loss, act, mask):
    from anime_recommendations_amd.engine import TrainEngine
    U, A, ui, ai, t = _problem(13, 2000, 400, 3001)
    eng = TrainEngine(U.shape[0], A.shape[0], max_batch=512, arena_steps=4, loss=loss, activation=act,
                      metrics=mask)
    hv = dict(HEAD, mov_mean=0.05, mov_var=0.5)
    eng.set_head(**hv)
    eng.set_weights(U, A)
    dev = eng.device
    vu, va, vt = (torch.from_numpy(x).to(dev) for x in (ui, ai, t))
    logs = eng.eval_logs(vu, va, vt)
    acc, rec = eng.read_metric_acc("val"), eng.read_state()
    st = orc.new_state(U, A, orc.new_head(**hv))
    want = mr.evaluate(st, ui, ai, t, act, loss)
    _check_acc(acc, dict(n_seen=rec["val_n"]), want, mask, len(t))
    # evaluate keeps its return values; the logs carry them
    vl, vm = eng.evaluate(vu, va, vt)
    assert abs(logs["loss"] - vl) <= 1e-12 * abs(vl) and abs(logs["mse"] - vm) <= 1e-12 * vm
    again = eng.read_metric_acc("val")                                  # a second pass: the same bins
    assert again["auc_pos"].tobytes() == acc["auc_pos"].tobytes() and again["auc_neg"].tobytes() == acc["auc_neg"].tobytes()
    eng.close()


def test_c_entry_points_refuse_bad_masks_before_enqueueing():
    from anime_recommendations_amd import _lib
    from anime_recommendations_amd.engine import TrainEngine
    lib = _lib.load()
    U, A, ui, ai, t = _problem(14, 300, 200, 256)
    eng = TrainEngine(300, 200, max_batch=256, arena_steps=4, loss="mse", activation="linear", metrics=1)
    eng.set_epoch(ui, ai, t, [0], [256], [orc.adam_alpha(1e-5, 1)])
    eng.run(1, use_graph=False)
    eng.synchronize()
    h, acc = eng._trainer, _lib.ptr(eng.metric_acc)
    before = eng.read_metric_acc().tobytes()
    assert lib.anirec_trainer_set_metrics(h, 128, acc) == -1
    assert lib.anirec_trainer_set_metrics(h, 64, acc) == -1          # AUC on a linear head
    assert lib.anirec_trainer_set_metrics(h, 0, acc) == 0
    assert lib.anirec_trainer_set_metrics(h, 1, None) == 0            # NULL acc: no metrics
    u, a = (torch.from_numpy(x).to(eng.device).to(torch.int32) for x in (ui, ai))
    tt = torch.from_numpy(t).to(eng.device)
    args = (_lib.ptr(u), _lib.ptr(a), _lib.ptr(tt), 256, eng._sp())
    assert lib.anirec_eval_metrics(C_desc(eng), 64, acc, *args) == -1
    assert lib.anirec_eval_metrics(C_desc(eng), 1 << 9, acc, *args) == -1
    torch.cuda.synchronize()
    assert eng.read_metric_acc().tobytes() == before
    with pytest.raises(ValueError):
        TrainEngine(300, 200, max_batch=256, arena_steps=4, activation="tanh", metrics=64)
    eng.close()


def C_desc(eng):
    import ctypes
    return ctypes.byref(eng.desc)


# ---- two gloo ranks on cuda:0 against one GPU -------------------------------------------------------------------
def _dist_problem():
    U, A, ui, ai, t = _problem(21, 1501, 500, 7 * 2000 - 333)
    return U, A, ui, ai, t, np.random.default_rng(22).permutation(len(ui))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _epoch(eng, mode, world, rank, out_dir):
    from anime_recommendations_amd import schedule
    U, A, ui, ai, t, perm = _dist_problem()
    dev = eng.device
    eng.set_head(**HEAD)
    eng.set_weights(U, A)
    eng.reset_optimizer()
    tu, ta, tt, tp = (torch.from_numpy(np.asarray(x)).to(dev) for x in (ui, ai, t, perm))
    n_steps = (len(perm) + 1999) // 2000
    eng.set_epoch_global(tu, ta, tt, tp, schedule.step_rates("adam", 3e-5, 1, n_steps))
    eng.reset_metrics()
    eng.run(n_steps, use_graph=False)
    logs = eng.epoch_logs()
    val = eng.eval_logs(tu[:3000], ta[:3000], tt[:3000])
    if rank == 0:
        with open(os.path.join(out_dir, "%s_%d.json" % (mode, world)), "w") as f:
            json.dump(dict(train=logs, val=val), f)


def _dist_worker(rank, world, port, out_dir, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from anime_recommendations_amd.dist import DistTrainEngine
        U, A = _dist_problem()[:2]
        eng = DistTrainEngine(U.shape[0], A.shape[0], 2000 // world, l2=1e-4, arena_steps=4,
                              device=torch.device("cuda:0"), mode=mode, metrics=ALL)
        _epoch(eng, mode, world, rank, out_dir)
        eng.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["sharded", "replicated"])
def test_two_gloo_ranks_match_the_one_gpu_history_columns(tmp_path, mode):
    mp.spawn(_dist_worker, args=(1, _port(), str(tmp_path), mode), nprocs=1, join=True)
    mp.spawn(_dist_worker, args=(2, _port(), str(tmp_path), mode), nprocs=2, join=True)
    one = json.load(open(tmp_path / ("%s_1.json" % mode)))
    two = json.load(open(tmp_path / ("%s_2.json" % mode)))
    for part in ("train", "val"):
        assert set(one[part]) == set(two[part]) and "auc" in one[part]
        for k, v in one[part].items():
            assert abs(two[part][k] - v) <= 1e-5 * abs(v) + 2e-5, (part, k, v, two[part][k])


# ---- the neural_network component ---------------------------------------------------------------------------------
def test_neural_network_component_monitors_val_auc(tmp_path):
    import pandas as pd
    from anime_recommendations_amd import data, weights_io
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(tmp_path / "store"), ANIREC_SEED="3")
    paths = data.write_synthetic_dataset(str(tmp_path / "data"), n_users=200, n_anime=300, n_ratings=12_000, seed=4)
    reg = ("import sys; sys.path.insert(0, %r); from anime_recommendations_amd import artifacts; "
           "artifacts.log_artifact('user_stats.parquet', %r, 'parquet')" % (ROOT, paths["user_stats"]))
    subprocess.run([sys.executable, "-c", reg], env=env, check=True, timeout=300)
    nn = dict(test_size=1500, TPU_INIT=False, embedding_size=128, kernel_initializer="he_normal",
              activation_function="sigmoid", model_loss="binary_crossentropy", optimizer="Adam",
              start_lr=1e-4, min_lr=1e-4, max_lr=5e-4, batch_size=1500, rampup_epochs=2, sustain_epochs=0,
              exp_decay=0.8, weights_artifact="wandb_main_weights.h5", save_weights_only=True,
              checkpoint_metric="val_auc", save_freq="epoch", mode="max", save_best_weights=True, verbose=1,
              epochs=4, save_model=True, model_name="./wandb_anime_nn.h5",
              input_data="user_stats.parquet:latest", project_name="anime_recommendations",
              model_artifact="wandb_anime_nn.h5", history_csv="wandb_anime_nn_history.csv",
              ID_emb_name="user_embedding", anime_emb_name="anime_embedding", merged_name="dot_product",
              main_df_type="parquet", model_type="h5", history_type="history_csv", weights_type="h5",
              model_metrics='["mae","accuracy","AUC","RootMeanSquaredError"]', l2_reg_factor=1e-4)
    argv = [sys.executable, os.path.join(ROOT, "neural_network", "neural_network.py")]
    for k, v in nn.items():
        argv += ["--" + k, str(v)]
    r = subprocess.run(argv, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    csv = tmp_path / "wandb_anime_nn_history.csv"
    assert open(csv).readline().strip() == (",loss,mae,accuracy,auc,root_mean_squared_error,val_loss,val_mae,"
                                            "val_accuracy,val_auc,val_root_mean_squared_error,lr")
    hist = pd.read_csv(csv)
    assert len(hist) == 4 and np.isfinite(hist.to_numpy()).all()
    best = int(np.argmax(hist["val_auc"].to_numpy()))
    found = {}
    for dp, _, fs in os.walk(tmp_path / "store"):
        if "artifact.json" in fs:
            meta = json.load(open(os.path.join(dp, "artifact.json")))
            found[meta["name"]] = os.path.join(dp, meta["file"])
    m = weights_io.load_model(found["wandb_main_weights.h5"])
    # the weights file holds the best val_auc epoch: its validation metrics, restated, are that row of the History
    df = pd.read_parquet(paths["user_stats"])
    table = data.encode_frame(df)
    _, te = table.split(1500)
    vu, va, vt = (np.asarray(c[te]) for c in (table.user, table.anime, table.rating))
    st = orc.new_state(m["U"], m["A"], orc.new_head(**{k: m["head"][k] for k in
                                                      ("w", "b", "gamma", "beta", "mov_mean", "mov_var")}))
    v = mr.evaluate(st, vu, va, vt.astype(f32), "sigmoid").values()
    row = hist.iloc[best]
    assert abs(row["val_auc"] - v["auc"]) < 1e-5
    assert abs(row["val_mae"] - v["mae"]) < 1e-5 * v["mae"] + 1e-6
    assert abs(row["val_root_mean_squared_error"] - v["rmse"]) < 2e-6
    assert abs(row["val_accuracy"] - v["accuracy"]) <= (mr.evaluate(st, vu, va, vt.astype(f32), "sigmoid").near_half
                                                        / len(vt) + 1e-9)
