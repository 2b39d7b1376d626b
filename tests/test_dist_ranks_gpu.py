"""GPU tests of the multi-rank path at 3 and 8 ranks, with the REAL HIP step halves and inference ops.

Gloo ranks share cuda:0 (RCCL needs one GPU per rank), so these tests run on a one-GPU box; they are the evidence for
the rank counts the driver's 8-GPU node runs.  What only shows with more than two ranks:
  * the head kernel merging n_seg > 2 packets (some empty, some of one rating) in rank order;
  * user shards of different sizes (n_users % world != 0), gathered and re-interleaved tables and Adam slots;
  * the automatic lazy-user-rows choice, which must be the same on every rank when the shards straddle its threshold;
  * a rank with no rating in the epoch and no validation row (empty device columns);
  * replicated_rs row shards that are short or empty, and the user-sharded mode with fewer users than ranks;
  * query-sharded inference with shards of different sizes and empty ones.
Every training result is held to the oracle stepping on the global batches (world * batch_per_rank ratings) with the
tolerances of test_dist_gpu.py.  One spawn per (world, problem); the modes run one after another inside it.  At most
8 ranks at once, every process group with a 120 s collective timeout."""
import datetime
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metrics_restatement as mr
from oracle import anirec_oracle as orc

pytestmark = pytest.mark.gpu
f32 = np.float32
LR = 3e-5
TIMEOUT = datetime.timedelta(seconds=120)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _spawn(fn, world, *args):
    mp.spawn(fn, args=(world, _port()) + args, nprocs=world, join=True)


def _tables(rng, n_u, n_a):
    return (rng.uniform(-0.05, 0.05, (n_u, 128)).astype(f32), rng.uniform(-0.05, 0.05, (n_a, 128)).astype(f32))


# ---- training problems: dict(U, A, ui, ai, t, perm, bpr, n_val) as a function of the world size ---------------------
def _uniform(world):
    """3001 users (3001 % 3 == 3001 % 8 == 1: shards of different sizes), 11 global batches of about 2000: a full lazy
    window of 8, then a ragged last batch."""
    rng = np.random.default_rng(31)
    bpr = 2000 // world
    n_u, n_a, n = 3001, 700, 11 * bpr * world - 333
    U, A = _tables(rng, n_u, n_a)
    ui = rng.integers(0, n_u, n)
    ai = (rng.zipf(1.15, n) - 1) % n_a
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return dict(U=U, A=A, ui=ui, ai=ai, t=t, perm=rng.permutation(n), bpr=bpr, n_val=500)


# per-rank batch of the skewed problem: a whole global batch must fit ONE rank's max_batch (batch_slack(bpr))
_SKEW_BPR = {3: 20, 8: 3}


def _skew_shares(world):
    """Ratings per rank (user u belongs to rank u % world) of each of the 11 global batches."""
    Bg = world * _SKEW_BPR[world]
    even = lambda c, ranks: [c // len(ranks) + (i < c % len(ranks)) for i in range(len(ranks))]   # noqa: E731
    shares = [even(Bg, range(world)) for _ in range(10)] + [None]
    shares[3] = [Bg] + [0] * (world - 1)                        # only rank 0's users
    shares[6] = even(Bg - 1, range(world - 1)) + [1]            # rank G-1: exactly one rating
    half = (world + 1) // 2
    shares[8] = even(Bg, range(half)) + [0] * (world - half)    # about half the ranks empty
    shares[10] = [0] * (world - 1) + [Bg // 2 + 1]              # the ragged last batch on one rank
    return shares


def _skewed(world):
    from anime_recommendations_amd.dist import local_user_rows
    rng = np.random.default_rng(32)
    n_u, n_a = 3001, 700
    uo = []
    for sh in _skew_shares(world):
        u = np.concatenate([r + world * rng.integers(0, local_user_rows(n_u, r, world), c) for r, c in enumerate(sh)])
        uo.append(rng.permutation(u))
    uo = np.concatenate(uo)
    n = len(uo)
    U, A = _tables(rng, n_u, n_a)
    perm = rng.permutation(n)
    ui = np.empty(n, np.int64)
    ui[perm] = uo                                  # ui[perm[k Bg:(k + 1) Bg]] is batch k
    ai = (rng.zipf(1.15, n) - 1) % n_a
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return dict(U=U, A=A, ui=ui, ai=ai, t=t, perm=perm, bpr=_SKEW_BPR[world], n_val=500)


ABSENT = 1


def _absent(world):
    """No rating of the epoch (and so no validation row) belongs to rank ABSENT's users: its device columns are empty.
    Its users' ratings go to the neighbouring ranks, so the others carry about world / (world - 1) of a share."""
    rng = np.random.default_rng(33)
    bpr = 64
    n_u, n_a, n = 3001, 700, 11 * bpr * world - 50
    U, A = _tables(rng, n_u, n_a)
    ui = rng.integers(0, n_u, n)
    gone = ui % world == ABSENT
    ui[gone] += np.where(rng.random(gone.sum()) < 0.5, -1, 1)
    ai = (rng.zipf(1.15, n) - 1) % n_a
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return dict(U=U, A=A, ui=ui, ai=ai, t=t, perm=rng.permutation(n), bpr=bpr, n_val=500)


def _lazy_threshold(world):
    """2303 users on 3 ranks: local rows 768, 768, 767 against the automatic threshold 6 * batch_slack(64) = 768."""
    rng = np.random.default_rng(34)
    bpr = 64
    n_u, n_a, n = 2303, 700, 11 * bpr * world - 50
    U, A = _tables(rng, n_u, n_a)
    ui = rng.integers(0, n_u, n)
    ai = (rng.zipf(1.15, n) - 1) % n_a
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return dict(U=U, A=A, ui=ui, ai=ai, t=t, perm=rng.permutation(n), bpr=bpr, n_val=500)


def _tiny(world):
    """5 users and 12 anime on 8 ranks: replicated_rs shards of ceil(17 / 8) = 3 rows, rank 5's holds 2, ranks 6 and 7
    none; 5 validation rows, so ranks 5..7 of the replicated modes validate nothing; the user-sharded mode has ranks
    without a user."""
    rng = np.random.default_rng(35)
    bpr = 8
    n_u, n_a, n = 5, 12, 3 * bpr * world - 10
    U, A = _tables(rng, n_u, n_a)
    ui = rng.integers(0, n_u, n)
    ai = (rng.zipf(1.15, n) - 1) % n_a
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return dict(U=U, A=A, ui=ui, ai=ai, t=t, perm=rng.permutation(n), bpr=bpr, n_val=5)


_PROBLEMS = {"uniform": _uniform, "skewed": _skewed, "absent": _absent, "lazy_threshold": _lazy_threshold,
             "tiny": _tiny}


def _mode_args(mode):
    """mode name -> (DistTrainEngine mode, lazy); "sharded-lazy" forces the lazy user rows, "sharded-auto" leaves the
    choice to DistTrainEngine."""
    return {"sharded-lazy": ("sharded", True), "sharded-auto": ("sharded", None)}.get(mode, (mode, False))


def _train_worker(rank, world, port, out_dir, problem, modes, refused):
    """Trains ``problem`` in each of ``modes`` (and checks that each of ``refused`` raises ValueError on EVERY rank
    before any GPU work or collective); rank 0 writes <mode>.npz."""
    _init(rank, world, port)
    try:
        from anime_recommendations_amd import schedule
        from anime_recommendations_amd.dist import DistTrainEngine
        dev = torch.device("cuda:0")
        P = _PROBLEMS[problem](world)
        U, A, bpr, nv = P["U"], P["A"], P["bpr"], P["n_val"]
        for mode in refused:
            with pytest.raises(ValueError):
                DistTrainEngine(U.shape[0], A.shape[0], bpr, l2=1e-4, arena_steps=4, device=dev, mode=mode)
        tu, ta, tt, tp = (torch.from_numpy(np.asarray(P[k])).to(dev) for k in ("ui", "ai", "t", "perm"))
        n_steps = (len(P["perm"]) + world * bpr - 1) // (world * bpr)
        for mode in modes:
            m, lazy = _mode_args(mode)
            eng = DistTrainEngine(U.shape[0], A.shape[0], bpr, l2=1e-4, arena_steps=4, device=dev, mode=m, lazy=lazy)
            # the update path of the user rows is the same on every rank
            flags = [torch.zeros(1, dtype=torch.int32) for _ in range(world)]
            dist.all_gather(flags, torch.tensor([int(eng.eng.lazy)], dtype=torch.int32))
            lazies = [int(x) for x in flags]
            assert len(set(lazies)) == 1, (mode, lazies)
            if lazy is not None:
                assert eng.eng.lazy == lazy
            eng.set_head(w=1.2)
            eng.set_weights(U, A)
            eng.set_epoch_global(tu, ta, tt, tp, schedule.adam_alphas(LR, 1, n_steps))
            eng.reset_metrics()
            eng.run(n_steps)
            loss, mse = eng.epoch_metrics()
            vl, vm = eng.evaluate(tu[:nv], ta[:nv], tt[:nv])
            Ufull = eng.U.cpu().numpy()
            Aloc = eng.A.cpu()
            opt = eng.optimizer_state(iterations=n_steps)       # collective: the full-table Adam slots
            # replicas stay bit-identical: the anime table in every mode, the user table too when it is replicated
            for tbl in ([eng.A] if m == "sharded" else [eng.A, eng.eng.U]):
                tbl = tbl.cpu()
                a_all = [torch.empty_like(tbl) for _ in range(world)]
                dist.all_gather(a_all, tbl)
                assert all(torch.equal(x, a_all[0]) for x in a_all), mode
            if rank == 0:
                rec = eng.read_state()
                np.savez(os.path.join(out_dir, mode + ".npz"), U=Ufull, A=Aloc.numpy(), loss=loss, mse=mse, vl=vl,
                         vm=vm, w=rec["w"], gamma=rec["gamma"], beta=rec["beta"], mov_var=rec["mov_var"],
                         mU=opt["user_embedding/m"], vU=opt["user_embedding/v"], mA=opt["anime_embedding/m"],
                         vA=opt["anime_embedding/v"], lazy=lazies[0], n_local=eng.n_local)
            eng.close()
    finally:
        dist.destroy_process_group()


def _oracle(P, world):
    """The single-process oracle on the global batches: (state, loss of the epoch, val_loss, val_mse, steps)."""
    ui, ai, t, perm, nv = P["ui"], P["ai"], P["t"], P["perm"], P["n_val"]
    st = orc.new_state(P["U"], P["A"], orc.new_head(w=1.2))
    Bg = world * P["bpr"]
    losses, ns = [], []
    for k in range(0, len(perm), Bg):
        g = perm[k:k + Bg]
        met, _, _ = orc.train_step(st, ui[g], ai[g], t[g], LR)
        losses.append(float(met["loss"]) * len(g))
        ns.append(len(g))
    ev = orc.evaluate(st, ui[:nv], ai[:nv], t[:nv])
    return st, sum(losses) / sum(ns), float(ev["val_loss"]), float(ev["val_mse"]), len(ns)


def _check(d, ref):
    st, loss, vl, vm, steps = ref
    tol = LR * 2e-3 * steps
    np.testing.assert_allclose(d["U"], st["U"], atol=tol)
    np.testing.assert_allclose(d["A"], st["A"], atol=tol)
    # the gathered Adam slots (sharded: user rows re-interleaved; replicated_rs: every rank's row shard)
    for k in ("mU", "mA"):
        np.testing.assert_allclose(d[k], st[k], atol=2e-3 * max(np.abs(st[k]).max(), 1e-12), err_msg=k)
    for k in ("vU", "vA"):
        np.testing.assert_allclose(d[k], st[k], atol=4e-3 * max(np.abs(st[k]).max(), 1e-20), err_msg=k)
    h = st["head"]
    for k in ("w", "gamma", "beta"):
        assert abs(float(d[k]) - float(h[k])) < tol, k
    assert abs(float(d["mov_var"]) - float(h["mov_var"])) < 1e-6
    assert abs(float(d["loss"]) - loss) < 5e-6
    assert abs(float(d["vl"]) - vl) < 5e-6 and abs(float(d["vm"]) - vm) < 1e-6


def _run_and_check(tmp_path, problem, world, modes, refused=()):
    _spawn(_train_worker, world, str(tmp_path), problem, list(modes), list(refused))
    P = _PROBLEMS[problem](world)
    ref = _oracle(P, world)
    out = {}
    for mode in modes:
        d = np.load(tmp_path / (mode + ".npz"))
        _check(d, ref)
        out[mode] = d
    return out


@pytest.mark.parametrize("world", [3, 8])
def test_uneven_user_shards_match_oracle_in_every_mode(tmp_path, world):
    P = _uniform(world)
    assert len(P["U"]) % world != 0 and -(-len(P["perm"]) // (world * P["bpr"])) == 11
    _run_and_check(tmp_path, "uniform", world, ["sharded", "sharded-lazy", "replicated", "replicated_rs"])


@pytest.mark.parametrize("world", [3, 8])
def test_skewed_shares_match_oracle(tmp_path, world):
    """Global batches whose shares are all on rank 0, give rank G-1 one rating, leave about half the ranks empty, and
    (the ragged last one) lie on rank G-1 alone: the head kernel merges n_seg packets, empty ones skipped."""
    from anime_recommendations_amd.dist import batch_slack
    P = _skewed(world)
    Bg = world * P["bpr"]
    shares = [np.bincount(P["ui"][P["perm"][k:k + Bg]] % world, minlength=world) for k in range(0, len(P["perm"]), Bg)]
    assert [list(s) for s in shares] == _skew_shares(world)
    assert shares[8].tolist().count(0) >= world // 2 and shares[6][-1] == 1
    assert max(s.max() for s in shares) <= batch_slack(P["bpr"])      # every share fits a rank's max_batch
    _run_and_check(tmp_path, "skewed", world, ["sharded", "sharded-lazy"])


def test_rank_without_ratings_or_validation_rows_trains_and_evaluates(tmp_path):
    """Rank ABSENT's device columns of the epoch and of the validation slice are empty (no storage, a null pointer)."""
    world = 3
    P = _absent(world)
    assert not (P["ui"] % world == ABSENT).any()
    from anime_recommendations_amd.dist import batch_slack
    Bg = world * P["bpr"]
    assert max(np.bincount(P["ui"][P["perm"][k:k + Bg]] % world).max()
               for k in range(0, len(P["perm"]), Bg)) <= batch_slack(P["bpr"])
    _run_and_check(tmp_path, "absent", world, ["sharded", "sharded-lazy"])


def test_automatic_lazy_choice_is_the_same_on_every_rank(tmp_path):
    """lazy=None where the ranks' shards straddle the threshold (768, 768, 767 rows against 768): every rank takes
    the same update path (asserted in the worker) and the result is the oracle's."""
    from anime_recommendations_amd.dist import batch_slack, local_user_rows
    world, P = 3, _lazy_threshold(3)
    thr = 6 * batch_slack(P["bpr"])
    rows = [local_user_rows(len(P["U"]), r, world) for r in range(world)]
    assert rows == [thr, thr, thr - 1]
    out = _run_and_check(tmp_path, "lazy_threshold", world, ["sharded-auto"])
    assert int(out["sharded-auto"]["lazy"]) == 1          # decided from rank 0's (the largest) shard


def test_tiny_tables_on_eight_ranks(tmp_path):
    """Replicated tables of 17 rows on 8 ranks (replicated_rs: empty and short Adam row ranges; ranks without
    validation rows) train as the oracle; the user-sharded mode with 5 users refuses on every rank alike."""
    world = 8
    _run_and_check(tmp_path, "tiny", world, ["replicated", "replicated_rs"], refused=["sharded"])


# ---- metrics: the History columns of G gloo ranks equal the one-GPU run's --------------------------------------------
ALL = 127
HEAD = dict(w=1.2, b=0.05, gamma=0.9, beta=0.3)
_MET_BG = 1992                   # divisible by 3 and 8: the same global batches as the one-GPU run


def _metrics_problem():
    rng = np.random.default_rng(36)
    n_u, n_a, n = 1501, 500, 7 * _MET_BG - 333
    U, A = _tables(rng, n_u, n_a)
    ui = rng.integers(0, n_u, n)
    ai = (rng.zipf(1.15, n) - 1) % n_a
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return U, A, ui, ai, t, rng.permutation(n)


def _metrics_worker(rank, world, port, out_dir):
    _init(rank, world, port)
    try:
        from anime_recommendations_amd import _lib, schedule
        from anime_recommendations_amd.dist import DistTrainEngine
        from anime_recommendations_amd.engine import TrainEngine
        dev = torch.device("cuda:0")
        U, A, ui, ai, t, perm = _metrics_problem()
        tu, ta, tt, tp = (torch.from_numpy(np.asarray(x)).to(dev) for x in (ui, ai, t, perm))
        n_steps = (len(perm) + _MET_BG - 1) // _MET_BG
        rates = schedule.step_rates("adam", LR, 1, n_steps)
        out = {}
        if rank == 0:                           # the one-GPU run on the same global batches
            ref = TrainEngine(U.shape[0], A.shape[0], max_batch=_MET_BG, arena_steps=4, device=dev, metrics=ALL)
            ref.set_head(**HEAD)
            ref.set_weights(U, A)
            starts = np.arange(n_steps) * _MET_BG
            ref.set_epoch(tu[tp], ta[tp], tt[tp], starts, np.minimum(_MET_BG, len(perm) - starts), rates)
            ref.reset_metrics()
            ref.run(n_steps, use_graph=False)
            out["one"] = dict(train=ref.epoch_logs(), val=ref.eval_logs(tu[:3000], ta[:3000], tt[:3000]))
            ref.close()
        for mode in ("sharded", "replicated"):
            eng = DistTrainEngine(U.shape[0], A.shape[0], _MET_BG // world, l2=1e-4, arena_steps=4, device=dev,
                                  mode=mode, metrics=ALL)
            eng.set_head(**HEAD)
            eng.set_weights(U, A)
            eng.set_epoch_global(tu, ta, tt, tp, rates)
            eng.reset_metrics()
            eng.run(n_steps, use_graph=False)
            logs = eng.epoch_logs()
            val = eng.eval_logs(tu[:3000], ta[:3000], tt[:3000])
            # every rank's head covers the whole global batch: its train AUC bins hold every rating's unit mass
            acc = eng.eng.read_metric_acc("train")
            mass = int(acc["auc_pos"].sum()) + int(acc["auc_neg"].sum())
            assert mass == len(perm) * _lib.AUC_ONE, (mode, mass)
            out[mode] = dict(train=logs, val=val)
            eng.close()
        if rank == 0:
            with open(os.path.join(out_dir, "metrics.json"), "w") as f:
                json.dump(out, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [3, 8])
def test_history_columns_match_the_one_gpu_run(tmp_path, world):
    assert mr.ONE == 1 << 20
    _spawn(_metrics_worker, world, str(tmp_path))
    res = json.load(open(tmp_path / "metrics.json"))
    one = res["one"]
    for mode in ("sharded", "replicated"):
        for part in ("train", "val"):
            got = res[mode][part]
            assert set(got) == set(one[part]) and "auc" in got, (mode, part)
            for k, v in one[part].items():
                assert abs(got[k] - v) <= 1e-5 * abs(v) + 2e-5, (mode, part, k, v, got[k])


# ---- another optimiser: SGD, user-sharded, 3 ranks ----------------------------------------------------------------
def _sgd_problem():
    rng = np.random.default_rng(37)
    n_u, n_a, n = 1501, 500, 7 * 1998 - 333
    U, A = _tables(rng, n_u, n_a)
    ui = rng.integers(0, n_u, n)
    ai = (rng.zipf(1.15, n) - 1) % n_a
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return U, A, ui, ai, t, rng.permutation(n)


def _sgd_worker(rank, world, port, out_dir):
    _init(rank, world, port)
    try:
        from anime_recommendations_amd import schedule
        from anime_recommendations_amd.dist import DistTrainEngine
        dev = torch.device("cuda:0")
        U, A, ui, ai, t, perm = _sgd_problem()
        bpr = 1998 // world
        eng = DistTrainEngine(U.shape[0], A.shape[0], bpr, l2=1e-4, arena_steps=4, device=dev, mode="sharded",
                              optimizer="sgd")
        assert not eng.eng.lazy and eng.optimizer == "sgd"
        eng.set_head(w=1.2)
        eng.set_weights(U, A)
        eng.reset_optimizer()
        tu, ta, tt, tp = (torch.from_numpy(np.asarray(x)).to(dev) for x in (ui, ai, t, perm))
        n_steps = (len(perm) + 1997) // 1998
        eng.set_epoch_global(tu, ta, tt, tp, schedule.step_rates("sgd", LR, 1, n_steps))
        eng.reset_metrics()
        eng.run(n_steps)
        loss, _ = eng.epoch_metrics()
        Ufull = eng.U.cpu().numpy()
        opt = eng.optimizer_state(iterations=n_steps)
        if rank == 0:
            rec = eng.read_state()
            np.savez(os.path.join(out_dir, "sgd.npz"), U=Ufull, A=eng.A.cpu().numpy(), loss=loss, w=rec["w"],
                     gamma=rec["gamma"], beta=rec["beta"], mov_var=rec["mov_var"], keys=np.array(sorted(opt)))
        eng.close()
    finally:
        dist.destroy_process_group()


def test_sgd_user_sharded_on_three_ranks_matches_the_restatement(tmp_path):
    _spawn(_sgd_worker, 3, str(tmp_path))
    d = np.load(tmp_path / "sgd.npz")
    U, A, ui, ai, t, perm = _sgd_problem()
    st = orc.new_state(U, A, orc.new_head(w=1.2), optimizer="sgd")
    losses, ns = [], []
    for k in range(0, len(perm), 1998):
        g = perm[k:k + 1998]
        met, _, _ = orc.train_step(st, ui[g], ai[g], t[g], LR)
        losses.append(float(met["loss"]) * len(g))
        ns.append(len(g))
    tol = LR * 2e-3 * len(ns)
    np.testing.assert_allclose(d["U"], st["U"], atol=tol)
    np.testing.assert_allclose(d["A"], st["A"], atol=tol)
    assert "user_embedding/m" not in d["keys"].tolist() and "iterations" in d["keys"].tolist()
    h = st["head"]
    for k in ("w", "gamma", "beta"):
        assert abs(float(d[k]) - float(h[k])) < tol, k
    assert abs(float(d["mov_var"]) - float(h["mov_var"])) < 1e-6
    assert abs(float(d["loss"]) - sum(losses) / sum(ns)) < 5e-6


# ---- query-sharded inference on the HIP ops -------------------------------------------------------------------------
_INFER_N = (5, 203, 2500)
_PRED_HEAD = dict(orc.new_head(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4))


def _infer_tables(n):
    rng = np.random.default_rng(40 + n)
    W = rng.normal(0, 0.05, (n, 128)).astype(f32)
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    return W, keep


def _predict_tables():
    rng = np.random.default_rng(39)
    U = rng.normal(0, 0.05, (3000, 128)).astype(f32)
    A = rng.normal(0, 0.05, (700, 128)).astype(f32)
    return U, A


def _predict_queries(n):
    rng = np.random.default_rng(50 + n)
    users = rng.integers(0, 3000, n).astype(np.int32)
    watched = rng.integers(0, 2 ** 32, (n, (700 + 31) // 32), dtype=np.uint64).astype(np.uint32).view(np.int32)
    return users, watched


def _infer_worker(rank, world, port, out_dir):
    _init(rank, world, port)
    try:
        from anime_recommendations_amd import dist_infer, ops
        dev = torch.device("cuda:0")
        res = {}
        for n in _INFER_N:
            W, keep = _infer_tables(n)
            Wh = ops.rownorm(torch.from_numpy(W))
            k = min(10, n - 1)
            res["Wh_%d" % n] = [Wh.cpu().numpy()]
            for tag, kp in (("all", None), ("keep", keep if n == 203 else None)):
                if tag == "keep" and kp is None:
                    continue
                di, ds = dist_infer.sharded_cosine_topk(Wh, k, keep=kp)
                si, ss, _ = ops.cosine_topk_mfma(Wh, torch.arange(n, dtype=torch.int32, device=dev), k, keep=kp)
                res["cos_%s_%d" % (tag, n)] = [x.cpu().numpy() for x in (di, ds, si, ss)]
        U, A = (torch.from_numpy(x).to(dev) for x in _predict_tables())
        for n in _INFER_N:
            users, watched = _predict_queries(n)
            wb = watched if n == 203 else None
            di, dp = dist_infer.sharded_predict_topk(U, A, _PRED_HEAD, users, 10, wb)
            si, sp, _ = ops.predict_topk_mfma(U, A, _PRED_HEAD, users, 10, wb)
            res["pred_%d" % n] = [x.cpu().numpy() for x in (di, dp, si, sp)]
        torch.cuda.synchronize()
        if rank == 0:
            np.savez(os.path.join(out_dir, "infer.npz"),
                     **{"%s__%d" % (key, j): a for key, v in res.items() for j, a in enumerate(v)})
    finally:
        dist.destroy_process_group()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("world", [3, 8])
def test_sharded_inference_on_the_hip_ops_equals_the_single_process_call(tmp_path, world):
    """sharded_cosine_topk / sharded_predict_topk with the default MFMA ops, bitwise the single-process call over
    the whole query set: 5 queries (fewer than the ranks: empty shards), 203, 2500; one keep mask, one watched set."""
    from anime_recommendations_amd import dist_infer
    assert dist_infer.shard_bounds(5, world - 1, world)[1] - dist_infer.shard_bounds(5, world - 1, world)[0] \
        == (1 if world == 3 else 0)
    _spawn(_infer_worker, world, str(tmp_path))
    d = np.load(tmp_path / "infer.npz")
    keys = sorted({f.split("__")[0] for f in d.files if not f.startswith("Wh_")})
    assert len(keys) == 2 * len(_INFER_N) + 1
    for key in keys:
        di, ds, si, ss = (d["%s__%d" % (key, j)] for j in range(4))
        n = int(key.rsplit("_", 1)[1])
        assert di.shape == si.shape and di.shape[0] == n, key
        assert np.array_equal(di, si), key
        assert np.array_equal(_bits(ds), _bits(ss)), key
    # the cosine lists are the oracle's (every query of the small sizes, 150 of the large one)
    for n in _INFER_N:
        _, keep = _infer_tables(n)
        Wh = d["Wh_%d__0" % n]                      # the table the kernels ranked (ops.rownorm's)
        k = min(10, n - 1)
        qs = np.arange(n) if n < 1000 else np.random.default_rng(7).choice(n, 150, replace=False)
        for tag, mask in (("all", None), ("keep", keep.astype(bool) if n == 203 else None)):
            if tag == "keep" and mask is None:
                continue
            oi, _ = orc.cosine_topk(Wh, qs, k, mask=mask)
            assert np.array_equal(d["cos_%s_%d__0" % (tag, n)][qs], oi), (tag, n)
