"""GPU tests of ops.predict_rank / ops.seen_bits (anirec_predict_rank, anirec_seen_bits) and of the evaluate component.

The yardstick for ranks is the exact whole-ranking path, which exists without them: for target t,
``ops.predict_topk(U, A, head, [users[row_t]], k=n_anime, watched_bits = the user's mask with bit a_t cleared)``; the
position of a_t in that list must equal rank[t] and the list's rating there must equal p[t] bit for bit, for every
target.  Sizes are the smallest that cross an edge of the kernel: 64 targets per workgroup, 64-row anime tiles (a
slice of the anime table is one tile while the targets are few: 129 anime lie just past two slices), 32-bit mask
words, a 256-wide row walked as two 128-float slices."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import poison
import rank_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (32, 64, 128, 256)
TBLOCK = 64                      # targets per workgroup of k_rank_count
HEAD = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
ACTS = ("sigmoid", "linear", "tanh", "relu", "softplus")


def _tables(rng, n_users, n_anime, dim):
    U = rng.normal(size=(n_users, dim)).astype(np.float32)
    A = rng.normal(size=(n_anime, dim)).astype(np.float32)
    return U, A


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _by_whole_ranking(tU, tA, head, users, trow, tanime, wb):
    """(rank, p bits) of every target through ops.predict_topk(k = n_anime): one query per target, its user's mask
    with the target's own bit cleared"""
    from anime_recommendations_amd import ops
    n_a = tA.shape[0]
    users, trow, tanime = np.asarray(users), np.asarray(trow), np.asarray(tanime)
    m = np.zeros((len(trow), (n_a + 31) // 32), np.uint32) if wb is None else np.asarray(wb).view(np.uint32)[trow].copy()
    m[np.arange(len(trow)), tanime >> 5] &= ~(np.uint32(1) << (tanime & 31).astype(np.uint32))
    idx, p = ops.predict_topk(tU, tA, head, users[trow], n_a, m.view(np.int32))
    idx, p = idx.cpu().numpy(), p.cpu().numpy()
    pos = np.array([R.position(idx[t], tanime[t]) for t in range(len(trow))], np.int64)
    return pos, p[np.arange(len(trow)), pos].view(np.int32)


def _check(tU, tA, head, users, trow, tanime, wb, what=""):
    from anime_recommendations_amd import ops
    rank, p = ops.predict_rank(tU, tA, head, users, trow, tanime, None if wb is None else np.asarray(wb).view(np.int32))
    assert rank.dtype.is_signed and rank.shape == (len(trow),) and p.shape == (len(trow),)
    rank, p = rank.cpu().numpy(), p.cpu().numpy()
    want_rank, want_p = _by_whole_ranking(tU, tA, head, users, trow, tanime, wb)
    np.testing.assert_array_equal(rank, want_rank, err_msg=str(what))
    np.testing.assert_array_equal(p.view(np.int32), want_p, err_msg=str(what))
    return rank, p


def _targets(rng, n_users, n_anime, n_t):
    """n_t targets: several of one user, users without any, and — past one block of targets — the targets of user 0
    on both sides of the block edge"""
    with_targets = np.arange(n_users)[::2] if n_users > 2 else np.arange(n_users)
    trow = rng.choice(with_targets, n_t)
    if n_t > TBLOCK:
        trow[TBLOCK - 2:TBLOCK + 1] = 0
    return trow.astype(np.int64), rng.integers(0, n_anime, n_t).astype(np.int64)


@pytest.mark.parametrize("dim", WIDTHS)
def test_shape_edges_equal_whole_ranking(dim):
    rng = np.random.default_rng(dim)
    for n_anime in (1, 31, 33, 64, 65, 129, 300):
        for n_users, n_t in ((1, 1), (5, TBLOCK), (70, TBLOCK + 1)):
            U, A = _tables(rng, n_users + 3, n_anime, dim)
            users = rng.permutation(n_users + 3)[:n_users]                 # a list of users, not the first rows
            trow, tanime = _targets(rng, n_users, n_anime, n_t)
            wb = R.pack(rng.random((n_users, n_anime)) < 0.3) if (n_anime + n_users) % 2 else None
            _check(_cuda(U), _cuda(A), HEAD, users, trow, tanime, wb, (dim, n_anime, n_users, n_t))


@pytest.mark.parametrize("dim", (32, 128))
def test_masks(dim):
    rng = np.random.default_rng(7 + dim)
    n_users, n_anime = 5, 70                                               # the last word holds 6 anime
    U, A = _tables(rng, n_users, n_anime, dim)
    tU, tA = _cuda(U), _cuda(A)
    users = np.arange(n_users)
    w = rng.random((n_users, n_anime)) < 0.4
    w[1] = True                                                            # every anime watched
    wb = R.pack(w)
    wb[:, -1] |= np.uint32(0xFFFFFFC0)                                     # bits past n_anime: they must not count
    wb[1] = 0xFFFFFFFF
    trow = np.repeat(users, 14)
    tanime = np.tile(np.arange(0, 70, 5), n_users)
    own = w[trow, tanime]
    assert own.any() and not own.all()                                     # targets whose own bit is set, and not
    rank, _ = _check(tU, tA, HEAD, users, trow, tanime, wb)
    assert (rank[trow == 1] == 0).all()                                    # only the target itself is eligible
    want, _ = R.ranks(_grid(tU, tA, HEAD, users), trow, tanime, w)
    np.testing.assert_array_equal(rank, want)                              # ... and the restatement on the exact grid
    rank0, _ = _check(tU, tA, HEAD, users, trow, tanime, None)
    assert (rank0 >= rank).all() and (rank0 > rank).any()


def _grid(tU, tA, head, users):
    from anime_recommendations_amd import ops
    return ops.predict_grid(tU, tA, head, users).cpu().numpy()


def _all_targets(n_users, n_anime):
    return np.repeat(np.arange(n_users), n_anime), np.tile(np.arange(n_anime), n_users)


@pytest.mark.parametrize("dim", (64, 128, 256))
def test_ties_and_odd_values(dim):
    rng = np.random.default_rng(11 + dim)
    n_users, n_anime = 3, 67
    U, A = _tables(rng, n_users, n_anime, dim)
    A[5] = A[40]
    A[66] = A[40]                                                          # duplicated rows: ties go by index
    A[64] = A[2]
    A[9] = 0                                                               # a zero row: cosine 0 with everyone
    A[13, dim // 2] = np.nan                                               # a NaN row: after every number
    A[50, 0] = np.nan
    U[2, 3] = np.nan                                                       # a NaN user: every rating NaN
    tU, tA = _cuda(U), _cuda(A)
    users = np.arange(n_users)
    trow, tanime = _all_targets(n_users, n_anime)
    wb = R.pack(rng.random((n_users, n_anime)) < 0.2)
    heads = {"plain": HEAD,
             "saturated": dict(HEAD, w=1e4),                              # sigmoid 0 or 1 almost everywhere
             "negative": dict(HEAD, w=-1.3),                              # hs < 0
             "flat": dict(HEAD, w=0.0)}                                   # hs = 0: one rating for all
    for name, head in heads.items():
        for mask in (None, wb):
            rank, p = _check(tU, tA, head, users, trow, tanime, mask, (dim, name))
            # every (user, anime) pair is a target, so p is the whole grid: the restatement of the definition on it
            want, _ = R.ranks(p.reshape(n_users, n_anime), trow, tanime, None if mask is None else R.unpack(mask, n_anime))
            np.testing.assert_array_equal(rank, want, err_msg=name)
            if mask is None:
                r2, p0 = rank.reshape(n_users, n_anime), p[:n_anime]
                assert all(sorted(r2[u]) == list(range(n_anime)) for u in range(n_users))   # a permutation per user
                assert r2[2].tolist() == list(range(n_anime))              # all NaN: by index
                assert np.isnan(p0[[13, 50]]).all() and r2[0, 13] == n_anime - 2 and r2[0, 50] == n_anime - 1
                if name == "flat":
                    assert np.unique(p0[~np.isnan(p0)]).size == 1
                if name == "saturated":
                    assert np.unique(p0[~np.isnan(p0)]).size <= 20        # 0 or 1 but for cosines within ~1e-3 of 0
                if name in ("plain", "negative"):
                    assert r2[0, 5] + 1 == r2[0, 40] == r2[0, 66] - 1 and r2[0, 2] + 1 == r2[0, 64]
    # relu below its knee everywhere: every rating is 0 and ranks go by index
    relu = dict(w=0.5, b=-1.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0, activation="relu")
    rank, p = _check(tU, tA, relu, users[:2], trow[:2 * n_anime], tanime[:2 * n_anime], None, (dim, "relu"))
    assert (p[~np.isnan(p)] == 0).all() and not np.isnan(p.reshape(2, n_anime)[:, :13]).any()
    assert rank.reshape(2, n_anime)[:, :13].tolist() == [list(range(13))] * 2
    want, _ = R.ranks(p.reshape(2, n_anime), trow[:2 * n_anime], tanime[:2 * n_anime])
    np.testing.assert_array_equal(rank, want)
    for act in ACTS:
        for mask in (None, wb):
            _check(tU, tA, dict(HEAD, activation=act), users, trow, tanime, mask, (dim, act))


@pytest.mark.parametrize("dim", (128, 256))
def test_results_do_not_depend_on_stale_memory(dim):
    """outputs, error word and workspace come from torch.empty: whatever they held, the ranks are the same"""
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(5 + dim)
    n_users, n_anime, n_t = 9, 129, TBLOCK + 1
    U, A = _tables(rng, n_users, n_anime, dim)
    tU, tA = _cuda(U), _cuda(A)
    users = np.arange(n_users)
    trow, tanime = _targets(rng, n_users, n_anime, n_t)
    wb = R.pack(rng.random((n_users, n_anime)) < 0.3)
    base_r, base_p = _check(tU, tA, HEAD, users, trow, tanime, wb)
    tu, ta = rng.integers(0, n_users, 500), rng.integers(0, n_anime, 500)
    base_bits = ops.seen_bits(tu, ta, n_users, n_anime).cpu().numpy()
    for byte in poison.ORDER:
        log = []
        with poison.poisoned(byte, log):
            rank, p = ops.predict_rank(tU, tA, HEAD, users, trow, tanime, wb.view(np.int32))
            bits = ops.seen_bits(tu, ta, n_users, n_anime)
        assert len(log) >= 6 and max(log) >= (n_users + n_anime) * dim * 4       # outputs, error words, workspace
        np.testing.assert_array_equal(rank.cpu().numpy(), base_r, err_msg=hex(byte))
        np.testing.assert_array_equal(p.cpu().numpy().view(np.int32), base_p.view(np.int32), err_msg=hex(byte))
        np.testing.assert_array_equal(bits.cpu().numpy(), base_bits, err_msg=hex(byte))


def test_two_calls_give_identical_bytes():
    """many slices of the anime table per target (their counts meet in atomic adds): run to run the same bytes, and
    the whole ranking's"""
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(21)
    n_users, n_anime, n_t = 40, 3000, 200
    U, A = _tables(rng, n_users, n_anime, 128)
    tU, tA = _cuda(U), _cuda(A)
    users = np.arange(n_users)
    trow, tanime = _targets(rng, n_users, n_anime, n_t)
    wb = R.pack(rng.random((n_users, n_anime)) < 0.1)
    r1, p1 = _check(tU, tA, HEAD, users, trow, tanime, wb)
    r2, p2 = ops.predict_rank(tU, tA, HEAD, users, trow, tanime, wb.view(np.int32))
    assert r1.tobytes() == r2.cpu().numpy().tobytes() and p1.tobytes() == p2.cpu().numpy().tobytes()


@pytest.mark.parametrize("n_anime", (31, 32, 33))
def test_seen_bits_equal_numpy(n_anime):
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(n_anime)
    n_users, n = 70, 3000                                                  # 3000 ratings of 70 x 33 pairs: repeats
    u, a = rng.integers(0, n_users, n), rng.integers(0, n_anime, n)
    got = ops.seen_bits(u, a, n_users, n_anime)
    assert got.dtype.is_signed and tuple(got.shape) == (n_users, (n_anime + 31) // 32)
    want = np.zeros((n_users, (n_anime + 31) // 32), np.uint32)
    np.bitwise_or.at(want, (u, a >> 5), np.uint32(1) << (a & 31).astype(np.uint32))
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(want, R.seen_bits(u, a, n_users, n_anime))
    assert not ops.seen_bits(u[:0], a[:0], n_users, n_anime).any()          # no rating: a zeroed table
    for bad_u, bad_a in ((n_users, 0), (-1, 0), (0, n_anime), (0, -1)):
        with pytest.raises(ValueError, match="out of range"):
            ops.seen_bits(np.append(u, bad_u), np.append(a, bad_a), n_users, n_anime)


def test_bad_targets_raise_and_leave_the_others_alone():
    import torch
    from anime_recommendations_amd import _lib, ops
    rng = np.random.default_rng(3)
    n_users, n_anime, dim = 5, 33, 64
    U, A = _tables(rng, n_users, n_anime, dim)
    tU, tA = _cuda(U), _cuda(A)
    users = np.arange(n_users)
    trow, tanime = _all_targets(n_users, n_anime)
    good_r, good_p = _check(tU, tA, HEAD, users, trow, tanime, None)
    for t, (br, ba) in ((0, (n_users, 0)), (70, (-1, 3)), (164, (2, n_anime)), (100, (2, -1))):
        r, a = trow.copy(), tanime.copy()
        r[t], a[t] = br, ba
        with pytest.raises(ValueError, match="out of range"):
            ops.predict_rank(tU, tA, HEAD, users, r, a)
    with pytest.raises(ValueError, match="out of range"):
        ops.predict_rank(tU, tA, HEAD, [0, 7], [0], [0])                   # a user the table does not hold
    with pytest.raises(ValueError):
        ops.predict_rank(tU, tA, HEAD, [], [0], [0])                       # a target and no user
    rank, p = ops.predict_rank(tU, tA, HEAD, users, [], [])
    assert rank.numel() == 0 and p.numel() == 0
    # the call after a refused one is unaffected
    rank, p = ops.predict_rank(tU, tA, HEAD, users, trow, tanime)
    assert np.array_equal(rank.cpu().numpy(), good_r) and np.array_equal(p.cpu().numpy().view(np.int32), good_p.view(np.int32))
    # the library call itself: the bad targets get -1 / NaN, the error word is set, the others are as they were
    lib = _lib.load()
    r, a = trow.copy(), tanime.copy()
    bad = [0, 70, 100, 164]
    r[0], a[70], r[100], a[164] = n_users, -1, -1, n_anime
    tr, ta, tus = _cuda(r.astype(np.int32)), _cuda(a.astype(np.int32)), _cuda(users.astype(np.int32))
    out_r = torch.full((len(r),), 99, dtype=torch.int32, device="cuda")
    out_p = torch.full((len(r),), 99.0, dtype=torch.float32, device="cuda")
    err = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.anirec_predict_rank_workspace_bytes(n_anime, n_users, len(r), dim), dtype=torch.uint8, device="cuda")
    h = _lib.Head(*(HEAD[k] for k in ("w", "b", "gamma", "beta", "mov_mean", "mov_var")))
    call = lambda n_t, dim_=dim: lib.anirec_predict_rank(
        _lib.ptr(tU), _lib.ptr(tA), dim_, n_anime, _lib.ptr(tus), n_users, ctypes.byref(h), 0, None, _lib.ptr(tr), _lib.ptr(ta),
        n_t, _lib.ptr(out_r), _lib.ptr(out_p), _lib.ptr(err), _lib.ptr(ws), ws.numel(), ctypes.c_void_p(0))
    _lib.check(call(len(r)))
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    gr, gp = out_r.cpu().numpy(), out_p.cpu().numpy()
    assert (gr[bad] == -1).all() and np.isnan(gp[bad]).all()
    ok = np.ones(len(r), bool)
    ok[bad] = False
    assert np.array_equal(gr[ok], good_r[ok]) and np.array_equal(gp[ok].view(np.int32), good_p[ok].view(np.int32))
    _lib.check(call(60))                                                   # targets 1..59 are fine, 0 is not
    assert int(err.item()) == 1
    tr[0] = 0
    _lib.check(call(60))
    assert int(err.item()) == 0                                            # the error word is cleared by the call
    assert call(60, 48) != 0 and call(60, 0) != 0                          # a width the kernels do not implement
    assert lib.anirec_predict_rank(_lib.ptr(tU), _lib.ptr(tA), dim, n_anime, _lib.ptr(tus), n_users, ctypes.byref(h), 0, None,
                                   _lib.ptr(tr), _lib.ptr(ta), 60, _lib.ptr(out_r), _lib.ptr(out_p), _lib.ptr(err),
                                   _lib.ptr(ws), ws.numel() - 1, ctypes.c_void_p(0)) == -3    # ANIREC_EWORKSPACE


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_frame_finds_planted_targets():
    """U and A built so that each held-out anime is its user's nearest row — next to a duplicate of it with a lower
    index that the user has a TRAINING rating for: hit_rate@1 == 1.0 only with the targets, the users and the masks
    wired to the right rows"""
    from anime_recommendations_amd import components as C, data
    rng = np.random.default_rng(17)
    n_users, n_anime, dim = 50, 40, 32
    A = rng.normal(size=(n_anime, dim)).astype(np.float32)
    A[:20] = A[20:]                                                        # anime j and j + 20 share a row
    target = 20 + rng.permutation(n_users) % 20                            # one held-out anime per user, in 20..39
    U = A[target] + 0.01 * rng.normal(size=(n_users, dim)).astype(np.float32)
    tr_u = np.concatenate([np.arange(n_users), rng.integers(0, n_users, 300)])
    tr_a = np.concatenate([target - 20, rng.integers(0, 20, 300)])         # the duplicate is watched; others in 0..19
    order = rng.permutation(n_users)
    low = np.arange(n_users) % 5 == 0                                      # ten held-out rows rated below min_rating
    table = data.RatingTable(np.concatenate([tr_u, order]), np.concatenate([tr_a, target[order]]),
                             np.concatenate([rng.integers(0, 11, len(tr_u)) / 10.0, np.where(low, 0.3, 0.9)]),
                             np.arange(n_users) * 3 + 7, np.arange(n_anime) * 2 + 1)
    model = dict(U=U, A=A, head=HEAD, user_ids=table.user_ids, anime_ids=table.anime_ids, activation="sigmoid")
    frame, summary = C.evaluate_frame(model, table, n_users, [1, 5], 0.5)
    assert summary["n"] == 40 and summary["n_users"] == 40
    assert frame["hit_rate"].tolist() == [1.0, 1.0] and frame["ndcg"].tolist() == [1.0, 1.0]
    assert summary["mrr"] == 1.0 and summary["mean_rank"] == 0.0
    # without the training ratings as a mask the duplicate comes first
    nothing = data.RatingTable(table.user[-n_users:], table.anime[-n_users:], table.rating[-n_users:], table.user_ids,
                               table.anime_ids)
    nothing = data.RatingTable(np.concatenate([[0], nothing.user]), np.concatenate([[39], nothing.anime]),
                               np.concatenate([[0.0], nothing.rating]), table.user_ids, table.anime_ids)
    frame, summary = C.evaluate_frame(model, nothing, n_users, [1, 5], 0.5)
    assert frame["hit_rate"].tolist() == [0.0, 1.0] and summary["mean_rank"] == 1.0


def _run(comp, flags, cwd, env):
    argv = [sys.executable, os.path.join(ROOT, comp, comp + ".py")]
    for k, v in flags.items():
        argv += ["--" + k, str(v)]
    r = subprocess.run(argv, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    return r.returncode, r.stdout.decode()


def test_evaluate_component_end_to_end(tmp_path):
    from anime_recommendations_amd import artifacts, components as C, data, recs, weights_io
    work = tmp_path
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(work / "store"), ANIREC_SEED="3")
    old = os.environ.get("ANIREC_ARTIFACT_DIR")
    os.environ["ANIREC_ARTIFACT_DIR"] = env["ANIREC_ARTIFACT_DIR"]
    try:
        paths = data.write_synthetic_dataset(str(work / "data"), n_users=200, n_anime=300, n_ratings=12_000)
        artifacts.log_artifact("user_stats.parquet", paths["user_stats"], "parquet")
        nn = dict(test_size=1000, TPU_INIT=False, embedding_size=64, kernel_initializer="he_normal",
                  activation_function="sigmoid", model_loss="binary_crossentropy", optimizer="Adam",
                  start_lr=1e-3, min_lr=1e-3, max_lr=5e-3, batch_size=1000, rampup_epochs=1, sustain_epochs=0,
                  exp_decay=0.8, weights_artifact="wandb_main_weights.h5", save_weights_only=True,
                  checkpoint_metric="val_loss", save_freq="epoch", mode="min", save_best_weights=True, verbose=0,
                  epochs=2, save_model=True, model_name="./wandb_anime_nn.h5",
                  input_data="user_stats.parquet:latest", project_name="anime_recommendations",
                  model_artifact="wandb_anime_nn.h5", history_csv="wandb_anime_nn_history.csv",
                  ID_emb_name="user_embedding", anime_emb_name="anime_embedding", merged_name="dot_product",
                  main_df_type="parquet", model_type="h5", history_type="history_csv", weights_type="h5",
                  model_metrics='["mse"]', l2_reg_factor=1e-4)
        code, out = _run("neural_network", nn, str(work), env)
        assert code == 0, out[-3000:]
        ks = [1, 5, 10, 50]
        ev = dict(input_data="user_stats.parquet:latest", main_df_type="parquet", model="wandb_anime_nn.h5:latest",
                  model_type="h5", project_name="anime_recommendations", test_size=1000, eval_k=str(ks), min_rating=0.7,
                  eval_csv="ranking_metrics.csv", eval_type="eval_csv", ID_emb_name="user_embedding",
                  anime_emb_name="anime_embedding")
        code, out = _run("evaluate", ev, str(work), env)
        assert code == 0, out[-3000:]
        summary = json.loads(out.strip().splitlines()[-1])
        frame = pd.read_csv(work / "ranking_metrics.csv", float_precision="round_trip")   # the float64 figures, bit for bit
        assert frame.columns.tolist() == ["k", "hit_rate", "ndcg"] and frame["k"].tolist() == ks
        assert frame["hit_rate"].between(0, 1).all() and (np.diff(frame["hit_rate"]) >= 0).all()
        assert frame["ndcg"].between(0, 1).all() and (frame["ndcg"] <= frame["hit_rate"]).all()
        logged = pd.read_csv(artifacts.use_artifact("ranking_metrics.csv:latest", "eval_csv"), float_precision="round_trip")
        pd.testing.assert_frame_equal(logged, frame)
        # the held-out rows are the run's validation rows: the host encoding and shuffle give the same table
        table = data.load_user_stats(paths["user_stats"])
        _, te = table.split(1000)
        take = table.rating[te] >= 0.7
        assert summary["n"] == int(take.sum()) > 100 and summary["test_size"] == 1000
        # the same figures from ranks recomputed through the whole-ranking path
        m = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
        assert m["U"].shape == (table.n_users, 64)
        users, row, anime, train = C.held_out_targets(table, 1000, 0.7)
        seen = R.seen_bits(table.user[train], table.anime[train], table.n_users, table.n_anime)
        want_rank, _ = _by_whole_ranking(_cuda(m["U"]), _cuda(m["A"]), weights_io.model_head(m), users, row, anime,
                                         seen[users])
        want = recs.ranking_metrics(want_rank, ks)
        assert frame["hit_rate"].tolist() == [want["hit_rate"][k] for k in ks]
        assert frame["ndcg"].tolist() == [want["ndcg"][k] for k in ks]
        for key in ("mrr", "mean_rank", "median_rank", "n"):
            assert summary[key] == want[key], key
        assert summary["n_users"] == len(users) and summary["hit_rate@10"] == want["hit_rate"][10]
        # a failure exits non-zero with the reason in ./evaluate.log
        code, out = _run("evaluate", dict(ev, model="no_such_model.h5:latest"), str(work), env)
        assert code != 0 and "evaluate failed" in open(work / "evaluate.log").read()
    finally:
        if old is None:
            os.environ.pop("ANIREC_ARTIFACT_DIR", None)
        else:
            os.environ["ANIREC_ARTIFACT_DIR"] = old
