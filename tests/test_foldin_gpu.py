"""GPU tests of the fold-in of new users (anirec_fold_in, ops.fold_in, recs.fold_in_users, the new_user_recs component).

Yardstick: the float64 NumPy restatement (tests/foldin_restatement.py) on the inputs of tests/foldin_cases.py — a
97-anime table, one new user per list length 0, 1, 2, 4, 5, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65, 700.  The kernel walks
a list with 256 / (width / 4) lane groups per pass: 32, 16, 8 and 4 ratings per pass at widths 32, 64, 128 and 256;
the lengths hold each of those counts and one past it.  It stages nothing in LDS, so no other length changes its path.

Tolerance: rows within ROW_TOL = 2.51e-5 and losses within LOSS_TOL = 1.45e-6 of the float64 restatement: 8 x the
largest distance of the FLOAT32 restatement from it over the same inputs (3.14e-6 and 1.81e-7, measured on the CPU and
held by tests/test_foldin_cpu.py; foldin_cases says where the largest one sits and why).  The two cases that run
huber's linear branch and the binary_crossentropy clip (foldin_cases.FAR_CASES, losses of 1.5 to 12) carry their own
measured pair: 9.48e-7 and 1.15e-6, again x 8.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import foldin_cases as K
import foldin_restatement as F
import poison

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ("binary_crossentropy", "sigmoid")
NAN_BITS = 0x7FC00000


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _head(act, dim=128):
    return dict(K.head_for(act, dim), activation=act)


def _fold(dim, loss, act, steps, off=None, idx=None, t=None, init=None, lr=K.LR):
    """ops.fold_in on a case's table and head -> (rows, loss) as NumPy arrays"""
    from anime_recommendations_amd import ops
    A, _, off0, idx0, t0, init0 = K.case_inputs(dim, loss, act)
    off, idx, t, init = (off0 if off is None else off, idx0 if idx is None else idx, t0 if t is None else t,
                         init0 if init is None else init)
    rows, ls = ops.fold_in(_cuda(A), _head(act, dim), off, idx, t, init, lr=lr, steps=steps, l2=K.L2, loss=loss)
    return rows.cpu().numpy(), ls.cpu().numpy()


def _raw(dim, off, idx, t, init, steps, bufs=None, preset=None, act=0, loss=0):
    """anirec_fold_in itself on the default case's table: no wrapper check between the test and the kernel.  ``bufs``:
    (rows, loss, err, workspace) tensors to write into (fresh ones otherwise); ``preset``: a 32-bit word the flag word
    holds on entry.  Returns (status, rows, loss, err, workspace)."""
    import torch
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    A = _cuda(K.table(dim))
    n_new = len(off) - 1
    if bufs is None:
        bufs = (torch.empty(n_new, dim, dtype=torch.float32, device="cuda"),
                torch.empty(n_new, dtype=torch.float32, device="cuda"),
                torch.empty(1, dtype=torch.int32, device="cuda"),
                torch.empty(int(lib.anirec_fold_in_workspace_bytes(K.N_ANIME, n_new, dim)), dtype=torch.uint8, device="cuda"))
    rows, ls, err, ws = bufs
    if preset is not None:
        err.fill_(preset)
    d_off, d_idx, d_t, d_init = _cuda(np.asarray(off, np.int64)), _cuda(np.asarray(idx, np.int32)), \
        _cuda(np.asarray(t, np.float32)), _cuda(np.asarray(init, np.float32))
    alpha = _cuda(K.alphas(steps)) if steps else None
    h = ops._head_struct(K.HEAD)
    st = lib.anirec_fold_in(_lib.ptr(A), dim, K.N_ANIME, ctypes.byref(h), act, loss, K.L2, _lib.ptr(d_off), _lib.ptr(d_idx),
                            _lib.ptr(d_t), n_new, _lib.ptr(d_init), _lib.ptr(alpha), steps, _lib.ptr(rows), _lib.ptr(ls),
                            _lib.ptr(err), _lib.ptr(ws), ws.numel(), None)
    torch.cuda.synchronize()
    return st, rows, ls, err, ws


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- 1. parity with the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("dim,loss,act", K.CASES + K.FAR_CASES)
def test_parity_with_the_float64_restatement(dim, loss, act):
    ref = K.reference(dim, loss, act)
    init = K.case_inputs(dim, loss, act)[5]
    has = np.array(K.LENGTHS) > 0
    row_tol, loss_tol = K.tolerances(dim, loss, act)
    for steps in K.STEPS:
        rows, ls = _fold(dim, loss, act, steps)
        want_rows, want_ls = ref[steps]
        d_row = np.abs(rows.astype(np.float64) - want_rows).max()
        d_loss = np.abs(ls[has].astype(np.float64) - want_ls[has]).max()
        print("fold_in parity dim %d %s %s steps %d: row %.3g (tol %.3g) loss %.3g (tol %.3g)"
              % (dim, loss, act, steps, d_row, row_tol, d_loss, loss_tol))
        assert d_row <= row_tol and d_loss <= loss_tol
        assert np.array_equal(_bits(rows[~has]), _bits(init[~has])) and np.isnan(ls[~has]).all()   # n == 0
        if steps == 0:
            assert np.array_equal(_bits(rows), _bits(init))


def test_other_learning_rate_and_one_start_row():
    """lr = 0.001 with 8 steps, and ``init`` given as one row for every user"""
    from anime_recommendations_amd import schedule
    A, head, off, idx, t, init = K.case_inputs(64, *DEFAULT)
    one = np.tile(init[3], (len(K.LENGTHS), 1))
    rows, ls = _fold(64, *DEFAULT, 8, init=init[3], lr=0.001)
    res = F.fold_in_many(A, head, off, idx, t, one, schedule.adam_alphas(0.001, 1, 8), l2=K.L2)
    has = np.array(K.LENGTHS) > 0
    assert np.abs(rows - np.stack([r["row"] for r in res])).max() <= K.ROW_TOL
    assert np.abs(ls[has] - np.array([r["loss"] for r in res])[has]).max() <= K.LOSS_TOL


def test_wrapper_refuses_bad_arguments():
    from anime_recommendations_amd import ops
    A, head, off, idx, t, init = K.case_inputs(32, *DEFAULT)
    tA = _cuda(A)
    with pytest.raises(ValueError, match="loss"):
        ops.fold_in(tA, _head("sigmoid"), off, idx, t, init, loss="hinge")
    with pytest.raises(ValueError, match="activation"):
        ops.fold_in(tA, dict(K.HEAD, activation="gelu"), off, idx, t, init)
    with pytest.raises(ValueError, match="embedding_size"):
        ops.fold_in(_cuda(np.zeros((97, 48), np.float32)), _head("sigmoid"), off, idx, t, np.zeros((16, 48), np.float32))
    with pytest.raises(ValueError, match="steps"):
        ops.fold_in(tA, _head("sigmoid"), off, idx, t, init, steps=-1)
    with pytest.raises(ValueError, match="offsets"):
        ops.fold_in(tA, _head("sigmoid"), off[::-1].copy(), idx, t, init)
    bad = idx.copy()
    bad[40] = K.N_ANIME
    with pytest.raises(ValueError, match="out of range"):
        ops.fold_in(tA, _head("sigmoid"), off, bad, t, init, steps=2)
    rows, ls = ops.fold_in(tA, _head("sigmoid"), [0], [], [], np.zeros((0, 32), np.float32))       # no users
    assert rows.shape == (0, 32) and ls.shape == (0,)


# ---- 2. independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", K.WIDTHS)
def test_a_user_does_not_depend_on_the_call(dim):
    """the same users alone, in a batch of 300 in shuffled order, and twice on the same buffers: the same bits"""
    _, _, off, idx, t, init = K.case_inputs(dim, *DEFAULT)
    steps = 8
    n_u = len(K.LENGTHS)
    base_rows, base_ls = _fold(dim, *DEFAULT, steps)
    for j in range(n_u):                                                    # alone
        sl = slice(off[j], off[j + 1])
        rows, ls = _fold(dim, *DEFAULT, steps, off=np.array([0, off[j + 1] - off[j]]), idx=idx[sl], t=t[sl], init=init[j:j + 1])
        assert np.array_equal(_bits(rows[0]), _bits(base_rows[j])) and np.array_equal(_bits(ls), _bits(base_ls[j:j + 1])), j
    rng = np.random.default_rng(7)                                          # among 284 others, shuffled
    lens = np.concatenate([np.array(K.LENGTHS), rng.integers(0, 41, 300 - n_u)])
    lists = [(idx[off[j]:off[j + 1]], t[off[j]:off[j + 1]], init[j]) for j in range(n_u)]
    for n in lens[n_u:]:
        lists.append((rng.integers(0, K.N_ANIME, n).astype(np.int32), (rng.integers(0, 11, n) / 10).astype(np.float32),
                      (rng.standard_normal(dim) * 0.05).astype(np.float32)))
    order = rng.permutation(300)
    b_off = np.concatenate([[0], np.cumsum([len(lists[o][0]) for o in order])]).astype(np.int64)
    rows, ls = _fold(dim, *DEFAULT, steps, off=b_off, idx=np.concatenate([lists[o][0] for o in order]),
                     t=np.concatenate([lists[o][1] for o in order]), init=np.stack([lists[o][2] for o in order]))
    where = np.argsort(order)[:n_u]                                         # position of user j in the batch
    assert np.array_equal(_bits(rows[where]), _bits(base_rows)) and np.array_equal(_bits(ls[where]), _bits(base_ls))
    st, r1, l1, e1, ws = _raw(dim, off, idx, t, init, steps)                # twice on the same buffers
    assert st == 0
    first = (r1.clone(), l1.clone())
    st, r2, l2, e2, _ = _raw(dim, off, idx, t, init, steps, bufs=(r1, l1, e1, ws))
    assert st == 0 and int(e2.item()) == 0
    assert np.array_equal(_bits(first[0].cpu().numpy()), _bits(r2.cpu().numpy()))
    assert np.array_equal(_bits(first[1].cpu().numpy()), _bits(l2.cpu().numpy()))
    assert np.array_equal(_bits(r2.cpu().numpy()), _bits(base_rows))        # and the raw call is the wrapper's


# ---- 3. edges --------------------------------------------------------------------------------------------------
def test_repeats_zero_rows_and_a_zero_start_row():
    A, head, _, _, _, init = K.case_inputs(128, *DEFAULT)
    z = K.ZERO_ANIME
    lists = [([5, 5, 5, 40, 5], [0.9, 0.9, 0.1, 0.3, 0.9]),          # one anime four times, with two different ratings
             ([z, z, z], [0.2, 0.8, 1.0]),                            # nothing but the zero row: the L2 term alone moves u
             ([z, 17, 60], [0.5, 1.0, 0.0]),
             ([3, 88, 41, 12, 66, 5, 50, 7, 19], [0.0, 1.0, 0.9, 0.1, 1.0, 0.0, 0.8, 0.2, 1.0])]   # from a zero start row
    off = np.concatenate([[0], np.cumsum([len(a) for a, _ in lists])]).astype(np.int64)
    idx = np.concatenate([a for a, _ in lists]).astype(np.int32)
    t = np.concatenate([r for _, r in lists]).astype(np.float32)
    start = init[:4].copy()
    start[3] = 0
    for steps in (1, 8, 100):
        rows, ls = _fold(128, *DEFAULT, steps, off=off, idx=idx, t=t, init=start)
        assert np.isfinite(rows).all() and np.isfinite(ls).all()
        res = F.fold_in_many(A, head, off, idx, t, start, K.alphas(steps), l2=K.L2)
        for j in range(3):
            assert np.abs(rows[j] - res[j]["row"]).max() <= K.ROW_TOL and abs(ls[j] - res[j]["loss"]) <= K.LOSS_TOL, (steps, j)
    # the zero start row: ru = 1e6 by the max(., 1e-12) clamp, the first Adam step moves every element by about lr.
    # The sign of a gradient element that rounds to nothing is the arithmetic's to pick, so the row is held to the
    # properties, not to the restatement's elements: finite, moved, and a better fit than the start
    rows, ls = _fold(128, *DEFAULT, 100, off=off, idx=idx, t=t, init=start)
    l0 = _fold(128, *DEFAULT, 0, off=off, idx=idx, t=t, init=start)[1]
    assert np.isfinite(rows[3]).all() and np.abs(rows[3]).max() > 1e-3 and ls[3] < l0[3]


def _clean_and_broken(dim, steps=8):
    _, _, off, idx, t, init = K.case_inputs(dim, *DEFAULT)
    st, rows, ls, err, _ = _raw(dim, off, idx, t, init, steps, preset=0x7F7F7F7F)
    assert st == 0 and int(err.item()) == 0                                 # the flag word is overwritten, not or-ed
    return (off, idx, t, init), rows.cpu().numpy(), ls.cpu().numpy()


@pytest.mark.parametrize("dim", (32, 128))
def test_bad_index_and_decreasing_offsets_poison_one_user_only(dim):
    (off, idx, t, init), rows0, ls0 = _clean_and_broken(dim)
    n_u = len(K.LENGTHS)
    for what in ("index past the table", "negative index", "decreasing offsets"):
        o, i = off.copy(), idx.copy()
        if what == "index past the table":
            victims = [12]
            i[off[12] + 40] = K.N_ANIME                                     # in the 63-rating user's list
        elif what == "negative index":
            victims = [15]
            i[off[15] + 699] = -1                                           # the last rating of the 700
        else:
            victims = [8]                                                   # offsets[9] < offsets[8]: user 8's pair decreases;
            o[9] = off[8] - 3                                               # user 9 now spans user 8's ratings and its own
        for preset in (0, 0x7F7F7F7F):
            st, rows, ls, err, _ = _raw(dim, o, i, t, init, 8, preset=preset)
            assert st == 0 and int(err.item()) == 1, what
            rows, ls = rows.cpu().numpy(), ls.cpu().numpy()
            for v in victims:
                assert (_bits(rows[v]) == NAN_BITS).all() and _bits(ls[v:v + 1])[0] == NAN_BITS, what
            same = [j for j in range(n_u) if j not in victims and not (what == "decreasing offsets" and j == 9)]
            assert np.array_equal(_bits(rows[same]), _bits(rows0[same])) and np.array_equal(_bits(ls[same]), _bits(ls0[same])), what


@pytest.mark.parametrize("byte", poison.ORDER)
def test_dirty_workspace_and_outputs(byte):
    """the workspace, the outputs and the flag word hold ``byte`` in every byte on entry: the same results"""
    import torch
    from anime_recommendations_amd import _lib
    for dim in (32, 256):
        (off, idx, t, init), rows0, ls0 = _clean_and_broken(dim)
        log = []
        with poison.poisoned(byte, log):
            rows, ls = _fold(dim, *DEFAULT, 8)
        assert len(log) >= 4 and sum(log) >= K.N_ANIME * dim * 4            # rows, loss, flag word, workspace
        assert np.array_equal(_bits(rows), _bits(rows0)) and np.array_equal(_bits(ls), _bits(ls0))
        n_new = len(off) - 1
        nb = int(_lib.load().anirec_fold_in_workspace_bytes(K.N_ANIME, n_new, dim))
        bufs = (poison.fill(torch.empty(n_new, dim, dtype=torch.float32, device="cuda"), byte),
                poison.fill(torch.empty(n_new, dtype=torch.float32, device="cuda"), byte),
                poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), byte),
                poison.fill(torch.empty(nb, dtype=torch.uint8, device="cuda"), byte))
        st, rows, ls, err, _ = _raw(dim, off, idx, t, init, 8, bufs=bufs)
        assert st == 0 and int(err.item()) == 0
        assert np.array_equal(_bits(rows.cpu().numpy()), _bits(rows0)) and np.array_equal(_bits(ls.cpu().numpy()), _bits(ls0))


def test_short_workspace_is_refused_and_writes_nothing():
    import torch
    from anime_recommendations_amd import _lib
    _, _, off, idx, t, init = K.case_inputs(64, *DEFAULT)
    n_new = len(off) - 1
    nb = int(_lib.load().anirec_fold_in_workspace_bytes(K.N_ANIME, n_new, 64))
    bufs = (torch.full((n_new, 64), 7.0, device="cuda"), torch.full((n_new,), 7.0, device="cuda"),
            torch.full((1,), 7, dtype=torch.int32, device="cuda"), torch.zeros(nb - 1, dtype=torch.uint8, device="cuda"))
    st, rows, ls, err, _ = _raw(64, off, idx, t, init, 8, bufs=bufs)
    assert st == -1 and bool((rows == 7).all()) and bool((ls == 7).all()) and int(err.item()) == 7


# ---- 4. it does what it is for ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """the components' small synthetic table (tests/test_components_gpu.py) and a model trainer.fit trained on it"""
    from anime_recommendations_amd import data, trainer
    frame = data.synth_user_stats(n_users=300, n_anime=500, n_ratings=40_000, seed=2)
    table = data.encode_frame(frame)
    cfg = trainer.FitConfig(epochs=3, batch_size=2000, test_size=2000, start_lr=1e-4, max_lr=5e-4, min_lr=1e-4,
                            rampup_epochs=2, verbose=0, seed=3, arena_steps=8, patience=10)
    res = trainer.fit(table, cfg)
    return frame, table, res


def _without_users(table, res, out):
    """the model file's dict with the rows of the user indices ``out`` taken out of the table"""
    keep = np.setdiff1d(np.arange(table.n_users), out)
    return dict(U=res.U[keep], A=res.A, head={k: float(res.head[k]) for k in ("w", "b", "gamma", "beta", "mov_mean", "mov_var")},
                user_ids=np.asarray(table.user_ids)[keep], anime_ids=np.asarray(table.anime_ids), activation="sigmoid",
                loss="binary_crossentropy")


def test_folded_rows_fit_their_users(trained):
    """20 users leave the trained table and are folded in from their training ratings.  In float64, the loss at the
    folded row is below the loss at the start row, and above the float64 restatement's final loss by no more than the
    row tolerance carried through the loss: L is smooth here (sigmoid head), so L(u) - L(u') <= |grad L|_1 x
    max |u - u'| along the segment; the bound takes |grad L|_1 at both ends and max |u - u'| = ROW_TOL."""
    from anime_recommendations_amd import recs
    frame, table, res = trained
    out = np.arange(5, 300, 15)[:20]
    model = _without_users(table, res, out)
    n_train = len(table) - 2000
    tu, ta, tr = table.user[:n_train], table.anime[:n_train], table.rating[:n_train]
    take = np.isin(tu, out)
    new = pd.DataFrame({"user_id": np.asarray(table.user_ids)[tu[take]], "anime_id": np.asarray(table.anime_ids)[ta[take]],
                        "rating": tr[take]})
    folded = recs.fold_in_users(model, new)
    assert sorted(folded["ids"].tolist()) == sorted(np.asarray(table.user_ids)[out].tolist()) and folded["n_dropped"] == 0
    rows = folded["rows"].cpu().numpy()
    init = np.asarray(model["U"], np.float32).mean(axis=0, dtype=np.float32)
    hs, hb = F.head_affine_f32(model["head"])
    Ah = F.normalised_rows(model["A"], np.float64)
    alphas = K.alphas(recs.FOLD_STEPS, recs.FOLD_LR)
    off, idx, t = folded["offsets"], folded["anime_idx"], folded["rating"]
    for j in range(len(out)):
        sl = slice(off[j], off[j + 1])
        a, tt = Ah[idx[sl]], t[sl].astype(np.float64)
        L = lambda u: F.loss_and_grad(np.asarray(u, np.float64), a, tt, hs, hb, 1e-4, "binary_crossentropy", "sigmoid", np.float64)
        l_init, l_gpu, g_gpu = L(init)[0], *L(rows[j])[:2]
        ref = F.fold_in(model["A"], model["head"], idx[sl], t[sl], init, alphas, l2=1e-4)
        g_ref = L(ref["row"])[1]
        bound = K.ROW_TOL * (np.abs(g_gpu).sum() + np.abs(g_ref).sum())
        print("fold-in user %d: %d ratings, loss %.6f at the start row, %.6f folded (restatement %.6f, bound %.2g), row "
              "distance %.3g" % (j, off[j + 1] - off[j], l_init, l_gpu, ref["loss"], bound, np.abs(rows[j] - ref["row"]).max()))
        assert l_gpu < l_init
        assert l_gpu <= ref["loss"] + bound
        assert abs(float(folded["loss"][j]) - l_gpu) <= K.LOSS_TOL      # out_loss is the loss at the row returned


def test_fold_in_users_with_an_empty_frame(trained):
    """no new users: empty ids, rows, losses and watched bits, through the same calls (n_new == 0)"""
    from anime_recommendations_amd import recs
    frame, table, res = trained
    model = _without_users(table, res, np.array([3]))
    folded = recs.fold_in_users(model, frame.iloc[:0][["user_id", "anime_id", "rating"]])
    assert len(folded["ids"]) == 0 and folded["n_dropped"] == 0 and folded["offsets"].tolist() == [0]
    assert tuple(folded["rows"].shape) == (0, 128) and tuple(folded["loss"].shape) == (0,)
    assert tuple(folded["watched"].shape) == (0, (table.n_anime + 31) // 32)


# ---- 5. the component, end to end ------------------------------------------------------------------------------
def _run(comp, flags, cwd, env):
    argv = [sys.executable, os.path.join(ROOT, comp, comp + ".py")]
    for k, v in flags.items():
        argv += ["--" + k, str(v)]
    r = subprocess.run(argv, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_new_user_recs_component(trained, tmp_path, golden_dir):
    from anime_recommendations_amd import artifacts, data, ops, recs, weights_io
    frame, table, res = trained
    out = np.array([7, 120, 260])
    model = _without_users(table, res, out)
    new_ids = np.asarray(table.user_ids)[out]
    new = frame[frame.user_id.isin(new_ids)][["user_id", "anime_id", "rating"]].reset_index(drop=True)
    new = pd.concat([new, pd.DataFrame({"user_id": [int(new_ids[1])], "anime_id": [10 ** 7], "rating": [0.5]})])   # no such row
    old = frame[~frame.user_id.isin(new_ids)]
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(tmp_path / "store"))
    prev = os.environ.get("ANIREC_ARTIFACT_DIR")
    os.environ["ANIREC_ARTIFACT_DIR"] = env["ANIREC_ARTIFACT_DIR"]
    try:
        anime, syn = data.synth_anime_tables(np.sort(frame["anime_id"].unique()))
        paths = {k: str(tmp_path / k) for k in ("user_stats.parquet", "all_anime.csv", "synopses.csv", "new.parquet", "m.h5")}
        old.to_parquet(paths["user_stats.parquet"], index=False)
        anime.to_csv(paths["all_anime.csv"], index=False)
        syn.to_csv(paths["synopses.csv"], index=False)
        new.to_parquet(paths["new.parquet"], index=False)
        weights_io.save_model(paths["m.h5"], model["U"], model["A"], model["head"], model["user_ids"], model["anime_ids"],
                              activation="sigmoid", loss="binary_crossentropy")
        artifacts.log_artifact("user_stats.parquet", paths["user_stats.parquet"], "parquet")
        artifacts.log_artifact("all_anime.csv", paths["all_anime.csv"], "raw_data")
        artifacts.log_artifact("synopses.csv", paths["synopses.csv"], "raw_data")
        artifacts.log_artifact("wandb_anime_nn.h5", paths["m.h5"], "h5")
        user = int(new_ids[1])
        flags = dict(main_df="user_stats.parquet:latest", main_df_type="parquet", project_name="anime_recommendations",
                     anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopsis_df="synopses.csv:latest",
                     sypnopsis_df_type="raw_data", model="wandb_anime_nn.h5:latest", model_type="h5",
                     model_user_query=0, random_user=False, model_recs_fn="model_recs.csv", save_model_recs=True,
                     model_num_recs=10, anime_types='["TV", "Movie"]', specify_types=True,
                     model_genres='["Action", "Comedy", None]', specify_genres=True, model_ID_flow=False,
                     model_ID_conf=False, model_recs_type="csv", flow_ID="user_id.csv:latest", flow_ID_type="csv",
                     new_ratings=paths["new.parquet"], fold_steps=40, fold_lr=0.01, fold_neighbours=True, user_query=user)
        _run("new_user_recs", flags, str(tmp_path), env)
        folded_path = artifacts.use_artifact("folded_users.npz:latest")
    finally:
        if prev is None:
            os.environ.pop("ANIREC_ARTIFACT_DIR", None)
        else:
            os.environ["ANIREC_ARTIFACT_DIR"] = prev
    got = pd.read_csv(tmp_path / ("User_ID_%d_model_recs.csv" % user))
    fmt = json.load(open(os.path.join(golden_dir, "reference_output_formats.json")))["User_ID_153695_model_recs.csv"]
    assert got.columns.tolist() == fmt["columns"] and len(got) == fmt["n_rows"]
    assert (np.diff(got["Prediction"]) <= 0).all() and got["Prediction"].between(0, 1).all()
    assert got["Type"].isin(["TV", "Movie"]).all() and got["Genres"].str.contains("Action|Comedy").all()
    assert not (set(got["anime_id"]) & set(new[new.user_id == user].anime_id))              # nothing watched is listed
    near = pd.read_csv(tmp_path / ("User_%d.csv" % user))
    fmt = json.load(open(os.path.join(golden_dir, "reference_output_formats.json")))["User_153695_similar_users.csv"]
    assert near.columns.tolist() == fmt["columns"] and len(near) == 10 and (np.diff(near["similarity"]) <= 0).all()
    assert not (set(near["similar_users"]) & set(new_ids.tolist())) and set(near["similar_users"]) <= set(model["user_ids"].tolist())
    # folded_users.npz holds every user of the file, rows and losses as ops.fold_in gives them
    z = np.load(folded_path)
    ids, off, a_idx, rat, dropped = recs.fold_in_csr(new, model["user_ids"], model["anime_ids"])
    assert dropped == 1 and z["ids"].tolist() == ids.tolist() and set(ids.tolist()) == set(new_ids.tolist())
    init = np.asarray(model["U"], np.float32).mean(axis=0, dtype=np.float32)
    rows, ls = ops.fold_in(_cuda(model["A"]), dict(model["head"], activation="sigmoid"), off, a_idx, rat, init, lr=0.01,
                           steps=40, l2=1e-4, loss="binary_crossentropy")
    assert np.array_equal(_bits(z["rows"]), _bits(rows.cpu().numpy())) and np.array_equal(_bits(z["loss"]), _bits(ls.cpu().numpy()))
    # and the listed anime are the top of ops.predict_topk on that row under the same mask
    q = int(np.nonzero(ids == user)[0][0])
    grid = ops.predict_grid(rows, _cuda(model["A"]), dict(model["head"], activation="sigmoid"), [q]).cpu().numpy()[0]
    listed = np.array([int(np.nonzero(model["anime_ids"] == a)[0][0]) for a in got["anime_id"]])
    np.testing.assert_allclose(got["Prediction"].to_numpy(), grid[listed], atol=1e-6)
