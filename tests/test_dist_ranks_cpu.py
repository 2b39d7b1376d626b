"""CPU gloo tests of the multi-rank partition and step protocol at 3 and 8 ranks (test_dist_cpu.py runs 2): the HIP step
halves replaced by test_dist_cpu's NumPy stand-in, the result held to the single-process oracle on the global batches.
Problems: user shards of different sizes in every mode, skewed shares (a batch on rank 0 alone, one rating on the last
rank, half the ranks empty, a ragged last batch on one rank), a rank with no rating and no validation row, tables
smaller than the world (empty replicated_rs row shards; the user-sharded mode refused on every rank alike), and the
automatic lazy-user-rows choice where the ranks' shards straddle its threshold (agreement only)."""
import datetime
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from anime_recommendations_amd import schedule
from anime_recommendations_amd.dist import (DistTrainEngine, batch_slack, local_user_rows, partition_epoch,
                                             partition_epoch_replicated)
from oracle import anirec_oracle as orc
from test_dist_cpu import NumpyStageEngine, _free_port

f32 = np.float32
LR = 3e-5
TIMEOUT = datetime.timedelta(seconds=120)


class LazyStageEngine(NumpyStageEngine):
    """The stand-in with the lazy flag a TrainEngine would end up with: the given one, or with ``lazy=None`` the
    engine's automatic rule (its own user rows against 6 max_batches in dense_mode 1)."""

    def __init__(self, n_user_rows, n_anime_rows, max_batch, lazy=None, dense_mode=1, **kw):
        super().__init__(n_user_rows, n_anime_rows, max_batch, dense_mode=dense_mode, **kw)
        self.lazy = bool(n_user_rows >= 6 * max_batch if lazy is None else lazy) and dense_mode == 1


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _tables(rng, n_u, n_a):
    return (rng.uniform(-0.05, 0.05, (n_u, 128)).astype(f32), rng.uniform(-0.05, 0.05, (n_a, 128)).astype(f32))


def _columns(rng, n_u, n_a, n):
    return rng.integers(0, n_u, n), (rng.zipf(1.2, n) - 1) % n_a, (rng.integers(0, 11, n) / 10).astype(f32)


def _uniform(world):
    rng = np.random.default_rng(61)
    n_u, n_a, bpr = 61, 40, 16                     # 61 % 3 == 1, 61 % 8 == 5
    n = 3 * bpr * world - 7
    U, A = _tables(rng, n_u, n_a)
    ui, ai, t = _columns(rng, n_u, n_a, n)
    return dict(U=U, A=A, ui=ui, ai=ai, t=t, perm=rng.permutation(n), bpr=bpr, n_val=100)


_SKEW_BPR = {3: 20, 8: 3}                          # a whole global batch fits one rank's batch_slack(bpr)


def _skew_shares(world):
    Bg = world * _SKEW_BPR[world]
    even = lambda c, k: [c // k + (i < c % k) for i in range(k)]          # noqa: E731
    half = (world + 1) // 2
    return [even(Bg, world), [Bg] + [0] * (world - 1), even(Bg - 1, world - 1) + [1],
            even(Bg, half) + [0] * (world - half), [0] * (world - 1) + [Bg // 2 + 1]]


def _skewed(world):
    rng = np.random.default_rng(62)
    n_u, n_a = 61, 40
    uo = []
    for sh in _skew_shares(world):
        u = np.concatenate([r + world * rng.integers(0, local_user_rows(n_u, r, world), c) for r, c in enumerate(sh)])
        uo.append(rng.permutation(u))
    uo = np.concatenate(uo)
    n = len(uo)
    U, A = _tables(rng, n_u, n_a)
    perm = rng.permutation(n)
    ui = np.empty(n, np.int64)
    ui[perm] = uo
    _, ai, t = _columns(rng, n_u, n_a, n)
    return dict(U=U, A=A, ui=ui, ai=ai, t=t, perm=perm, bpr=_SKEW_BPR[world], n_val=100)


ABSENT = 1


def _absent(world):
    rng = np.random.default_rng(63)
    n_u, n_a, bpr = 61, 40, 16
    n = 3 * bpr * world - 7
    U, A = _tables(rng, n_u, n_a)
    ui, ai, t = _columns(rng, n_u, n_a, n)
    gone = ui % world == ABSENT
    ui[gone] += np.where(rng.random(gone.sum()) < 0.5, -1, 1)
    return dict(U=U, A=A, ui=ui, ai=ai, t=t, perm=rng.permutation(n), bpr=bpr, n_val=100)


def _tiny(world):
    rng = np.random.default_rng(64)
    n_u, n_a, bpr = 5, 12, 8
    n = 3 * bpr * world - 10
    U, A = _tables(rng, n_u, n_a)
    ui, ai, t = _columns(rng, n_u, n_a, n)
    return dict(U=U, A=A, ui=ui, ai=ai, t=t, perm=rng.permutation(n), bpr=bpr, n_val=5)


_PROBLEMS = {"uniform": _uniform, "skewed": _skewed, "absent": _absent, "tiny": _tiny}


def _check_partition(P, rank, world, mode, lu, la, starts, counts, gcounts):
    ui, ai, perm, Bg = P["ui"], P["ai"], P["perm"], world * P["bpr"]
    n_steps = -(-len(perm) // Bg)
    assert list(gcounts) == [Bg] * (n_steps - 1) + [len(perm) - Bg * (n_steps - 1)]
    assert len(counts) == n_steps and sum(counts) == len(lu)
    for k, (s, c) in enumerate(zip(starts, counts)):
        g = perm[k * Bg:(k + 1) * Bg]
        if mode == "sharded":                   # by owner of the user, local rows = u // world
            mine = g[ui[g] % world == rank]
            assert (lu[s:s + c].numpy() == ui[mine] // world).all()
        else:                                   # contiguous slices of the batch, global user rows
            lo, hi = -(-len(g) * rank // world), -(-len(g) * (rank + 1) // world)
            mine = g[lo:hi]
            assert (lu[s:s + c].numpy() == ui[mine]).all()
        assert c == len(mine) and (la[s:s + c].numpy() == ai[mine]).all()


def _worker(rank, world, port, out_dir, problem, modes, refused):
    _init(rank, world, port)
    try:
        P = _PROBLEMS[problem](world)
        U, A, bpr, nv = P["U"], P["A"], P["bpr"], P["n_val"]
        for mode in refused:                    # refused on EVERY rank, before any collective
            with pytest.raises(ValueError):
                DistTrainEngine(U.shape[0], A.shape[0], bpr, device="cpu", engine_factory=LazyStageEngine, mode=mode)
        tu, ta, tt, tp = (torch.from_numpy(np.asarray(P[k])) for k in ("ui", "ai", "t", "perm"))
        for mode in modes:
            part = partition_epoch if mode == "sharded" else partition_epoch_replicated
            lu, la, _, starts, counts, gcounts = part(tu, ta, tt, tp, bpr * world, rank, world)
            _check_partition(P, rank, world, mode, lu, la, starts, counts, gcounts)
            eng = DistTrainEngine(U.shape[0], A.shape[0], bpr, l2=1e-4, device="cpu", engine_factory=LazyStageEngine,
                                  mode=mode)
            assert eng.n_local == (local_user_rows(U.shape[0], rank, world) if mode == "sharded" else U.shape[0])
            eng.set_head(w=1.2)
            eng.set_weights(U, A)
            n_steps = len(counts)
            eng.set_epoch_global(tu, ta, tt, tp, schedule.adam_alphas(LR, 1, n_steps))
            eng.reset_metrics()
            eng.run(n_steps)
            loss, mse = eng.epoch_metrics()
            vl, vm = eng.evaluate(tu[:nv], ta[:nv], tt[:nv])
            Ufull = eng.U.numpy()
            for tbl in ([eng.A] if mode == "sharded" else [eng.A, eng.eng.U]):
                a_all = [torch.empty_like(tbl) for _ in range(world)]
                dist.all_gather(a_all, tbl.contiguous())
                assert all(torch.equal(x, a_all[0]) for x in a_all), mode
            if rank == 0:
                rec = eng.read_state()
                np.savez(os.path.join(out_dir, mode + ".npz"), U=Ufull, A=eng.A.numpy(), loss=loss, mse=mse, vl=vl,
                         vm=vm, w=rec["w"], gamma=rec["gamma"])
    finally:
        dist.destroy_process_group()


def _run_and_check(tmp_path, problem, world, modes, refused=()):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), problem, list(modes), list(refused)), nprocs=world,
             join=True)
    P = _PROBLEMS[problem](world)
    ui, ai, t, perm, nv, Bg = P["ui"], P["ai"], P["t"], P["perm"], P["n_val"], world * P["bpr"]
    st = orc.new_state(P["U"], P["A"], orc.new_head(w=1.2))
    losses, ns = [], []
    for k in range(0, len(perm), Bg):
        g = perm[k:k + Bg]
        met, _, _ = orc.train_step(st, ui[g], ai[g], t[g], LR)
        losses.append(float(met["loss"]) * len(g))
        ns.append(len(g))
    ev = orc.evaluate(st, ui[:nv], ai[:nv], t[:nv])
    tol = LR * 2e-3 * len(ns)
    for mode in modes:
        d = np.load(tmp_path / (mode + ".npz"))
        np.testing.assert_allclose(d["U"], st["U"], atol=tol, err_msg=mode)
        np.testing.assert_allclose(d["A"], st["A"], atol=tol, err_msg=mode)
        h = st["head"]
        assert abs(float(d["w"]) - float(h["w"])) < tol and abs(float(d["gamma"]) - float(h["gamma"])) < tol, mode
        assert abs(float(d["loss"]) - sum(losses) / sum(ns)) < 5e-6, mode
        assert abs(float(d["vl"]) - float(ev["val_loss"])) < 5e-6 and abs(float(d["vm"]) - float(ev["val_mse"])) < 1e-6


@pytest.mark.parametrize("world", [3, 8])
def test_uneven_user_shards_in_every_mode(tmp_path, world):
    assert 61 % world
    _run_and_check(tmp_path, "uniform", world, ["sharded", "replicated", "replicated_rs"])


@pytest.mark.parametrize("world", [3, 8])
def test_skewed_shares(tmp_path, world):
    P = _skewed(world)
    Bg = world * P["bpr"]
    shares = [np.bincount(P["ui"][P["perm"][k:k + Bg]] % world, minlength=world).tolist()
              for k in range(0, len(P["perm"]), Bg)]
    assert shares == _skew_shares(world) and max(map(max, shares)) <= batch_slack(P["bpr"])
    _run_and_check(tmp_path, "skewed", world, ["sharded"])


@pytest.mark.parametrize("world", [3, 8])
def test_rank_without_ratings_or_validation_rows(tmp_path, world):
    P = _absent(world)
    assert not (P["ui"] % world == ABSENT).any()
    _run_and_check(tmp_path, "absent", world, ["sharded"])


def test_tables_smaller_than_the_world(tmp_path):
    """17 rows on 8 ranks: replicated_rs row shards of 3, rank 5's short, ranks 6 and 7 empty; 5 validation rows; the
    user-sharded mode with 5 users raises the same ValueError on every rank."""
    rows, world = 5 + 12, 8
    sr = -(-rows // world)
    assert [max(0, min(rows, r * sr + sr) - min(rows, r * sr)) for r in range(world)] == [3, 3, 3, 3, 3, 2, 0, 0]
    _run_and_check(tmp_path, "tiny", world, ["replicated", "replicated_rs"], refused=["sharded"])


def _lazy_worker(rank, world, port, n_users, bpr, out_dir):
    _init(rank, world, port)
    try:
        eng = DistTrainEngine(n_users, 40, bpr, device="cpu", engine_factory=LazyStageEngine, mode="sharded")
        flags = [torch.zeros(1, dtype=torch.int32) for _ in range(world)]
        dist.all_gather(flags, torch.tensor([int(eng.eng.lazy)], dtype=torch.int32))
        assert len({int(x) for x in flags}) == 1, [int(x) for x in flags]
        if rank == 0:
            np.save(os.path.join(out_dir, "lazy.npy"), int(flags[0]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [3, 8])
def test_automatic_lazy_choice_agrees_across_ranks(tmp_path, world):
    """Shards of 768 and 767 rows against the threshold 6 * batch_slack(64) = 768: every rank takes one choice."""
    bpr = 64
    thr = 6 * batch_slack(bpr)
    n_users = world * thr - 1
    rows = [local_user_rows(n_users, r, world) for r in range(world)]
    assert rows[0] == thr and rows[-1] == thr - 1
    mp.spawn(_lazy_worker, args=(world, _free_port(), n_users, bpr, str(tmp_path)), nprocs=world, join=True)
    assert int(np.load(tmp_path / "lazy.npy")) == 1
