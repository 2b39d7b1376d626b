"""GPU tests of the fold-in of new anime above the kernel: recs.fold_in_anime, recs.append_anime, the two new_anime
frames of components and the new_anime component, on the small trained model of tests/test_foldin_gpu.py (300 users x
500 anime)."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import foldin_cases as K
import foldin_restatement as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_KEYS = ("w", "b", "gamma", "beta", "mov_mean", "mov_var")


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


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


def _without_anime(table, res, out):
    """the model file's dict with the rows of the anime indices ``out`` taken out of the table"""
    keep = np.setdiff1d(np.arange(table.n_anime), out)
    return dict(U=res.U, A=res.A[keep], head={k: float(res.head[k]) for k in HEAD_KEYS},
                user_ids=np.asarray(table.user_ids), anime_ids=np.asarray(table.anime_ids)[keep], activation="sigmoid",
                loss="binary_crossentropy")


def _most_rated(table, n, skip=0):
    """indices of the n anime with the most ratings after the ``skip`` most rated"""
    return np.sort(np.argsort(-np.bincount(table.anime, minlength=table.n_anime), kind="stable")[skip:skip + n])


@pytest.fixture(scope="module")
def folded_12(trained):
    """12 anime leave the trained table and are folded in from their training ratings"""
    from anime_recommendations_amd import recs
    frame, table, res = trained
    out = _most_rated(table, 36)[::3]
    model = _without_anime(table, res, out)
    n_train = len(table) - 2000
    tu, ta, tr = table.user[:n_train], table.anime[:n_train], table.rating[:n_train]
    take = np.isin(ta, out)
    new = pd.DataFrame({"user_id": np.asarray(table.user_ids)[tu[take]], "anime_id": np.asarray(table.anime_ids)[ta[take]],
                        "rating": tr[take]})
    return out, model, new, recs.fold_in_anime(model, new)


def test_folded_rows_fit_their_anime(trained, folded_12):
    """In float64, the loss at each folded row is below the loss at the start row, and above the float64 restatement's
    final loss (run at the call's step count) by no more than the row tolerance carried through the loss: the bound of
    tests/test_foldin_gpu.py::test_folded_rows_fit_their_users, |grad L|_1 at both ends x ROW_TOL."""
    from anime_recommendations_amd import recs
    frame, table, res = trained
    out, model, new, folded = folded_12
    assert sorted(folded["ids"].tolist()) == sorted(np.asarray(table.anime_ids)[out].tolist()) and folded["n_dropped"] == 0
    assert tuple(folded["rated"].shape) == (12, (table.n_users + 31) // 32)
    rows = folded["rows"].cpu().numpy()
    init = np.asarray(model["A"], np.float32).mean(axis=0, dtype=np.float32)
    hs, hb = F.head_affine_f32(model["head"])
    Uh = F.normalised_rows(model["U"], np.float64)
    alphas = K.alphas(recs.FOLD_STEPS, recs.FOLD_LR)
    off, idx, t = folded["offsets"], folded["user_idx"], folded["rating"]
    for j in range(len(out)):
        sl = slice(off[j], off[j + 1])
        u, tt = Uh[idx[sl]], t[sl].astype(np.float64)
        L = lambda a: F.loss_and_grad(np.asarray(a, np.float64), u, tt, hs, hb, 1e-4, "binary_crossentropy", "sigmoid", np.float64)
        l_init, l_gpu, g_gpu = L(init)[0], *L(rows[j])[:2]
        ref = F.fold_in(model["U"], model["head"], idx[sl], t[sl], init, alphas, l2=1e-4)
        g_ref = L(ref["row"])[1]
        bound = K.ROW_TOL * (np.abs(g_gpu).sum() + np.abs(g_ref).sum())
        print("fold-in anime %d: %d ratings, loss %.6f at the start row, %.6f folded (restatement %.6f, bound %.2g), row "
              "distance %.3g" % (j, off[j + 1] - off[j], l_init, l_gpu, ref["loss"], bound, np.abs(rows[j] - ref["row"]).max()))
        assert l_gpu < l_init
        assert l_gpu <= ref["loss"] + bound
        assert abs(float(folded["loss"][j]) - l_gpu) <= K.LOSS_TOL      # out_loss is the loss at the row returned
        # the bits ops.seen_bits sets: exactly the users whose ratings were fitted
        words = folded["rated"][j].cpu().numpy().view(np.uint32)
        rated = np.nonzero((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1)
        assert sorted((rated[0] * 32 + rated[1]).tolist()) == sorted(set(idx[sl].tolist()))


def test_fold_in_anime_with_an_empty_frame(trained):
    from anime_recommendations_amd import recs
    frame, table, res = trained
    model = _without_anime(table, res, np.array([3]))
    folded = recs.fold_in_anime(model, frame.iloc[:0][["user_id", "anime_id", "rating"]])
    assert len(folded["ids"]) == 0 and folded["n_dropped"] == 0 and folded["offsets"].tolist() == [0]
    assert tuple(folded["rows"].shape) == (0, 128) and tuple(folded["loss"].shape) == (0,)
    assert tuple(folded["rated"].shape) == (0, (table.n_users + 31) // 32)


def _tables(frame):
    from anime_recommendations_amd import components as C, data
    anime, syn = data.synth_anime_tables(np.sort(frame["anime_id"].unique()))
    return anime, syn


def _loaded(tmp_path, frame):
    """the synthetic all_anime.csv / synopses.csv as the components load them"""
    from anime_recommendations_amd import components as C
    anime, syn = _tables(frame)
    anime.to_csv(tmp_path / "all_anime.csv", index=False)
    syn.to_csv(tmp_path / "synopses.csv", index=False)
    return C.load_anime_df(str(tmp_path / "all_anime.csv")), C.load_synopses(str(tmp_path / "synopses.csv"))


def test_similar_frame_lists_trained_anime_and_honours_the_filters(trained, folded_12, tmp_path):
    from anime_recommendations_amd import components as C
    frame, table, res = trained
    out, model, new, folded = folded_12
    anime_df, syn_df = _loaded(tmp_path, frame)
    q = int(folded["ids"][4])
    names = dict(zip(anime_df.anime_id, anime_df.Name))
    trained_names = {names[int(a)] for a in model["anime_ids"]}
    new_names = {names[int(a)] for a in folded["ids"]}
    got, fn = C.new_anime_similar_frame(model, folded, anime_df, syn_df, q, 25)
    ref_cols = C.similar_anime_frame(model["A"], model["anime_ids"], anime_df, syn_df, names[int(model["anime_ids"][0])], 3)[0].columns
    assert got.columns.tolist() == ref_cols.tolist() and len(got) == 25 and fn == "Anime_ID_%d_similar.csv" % q
    assert (np.diff(got["Similarity"]) <= 0).all() and set(got["Name"]) <= trained_names and not set(got["Name"]) & new_names
    # the cosines are those of the rows
    A64 = F.normalised_rows(model["A"], np.float64)
    r64 = F.normalised_rows(folded["rows"].cpu().numpy()[4:5], np.float64)[0]
    pos = {names[int(a)]: i for i, a in enumerate(model["anime_ids"])}
    np.testing.assert_allclose(got["Similarity"].to_numpy(), A64[[pos[n] for n in got["Name"]]] @ r64, atol=1e-6)
    assert got["Similarity"].iloc[0] >= np.sort(A64 @ r64)[-1] - 1e-6
    got, _ = C.new_anime_similar_frame(model, folded, anime_df, syn_df, q, 10, types=["TV", "Movie"], genres=["Action", "Comedy"])
    assert len(got) and got["Type"].isin(["TV", "Movie"]).all() and got["Genres"].str.contains("Action|Comedy").all()
    assert set(got["Name"]) <= trained_names
    with pytest.raises(ValueError, match="not in the new ratings file"):
        C.new_anime_similar_frame(model, folded, anime_df, syn_df, int(model["anime_ids"][0]), 5)


def test_audience_frame_lists_users_who_have_not_rated(trained, folded_12):
    from anime_recommendations_amd import components as C
    out, model, new, folded = folded_12
    q = int(folded["ids"][7])
    got, fn = C.new_anime_audience_frame(model, folded, q, 20)
    assert got.columns.tolist() == ["user_id", "Prediction"] and len(got) == 20 and fn == "Anime_ID_%d_audience.csv" % q
    assert (np.diff(got["Prediction"]) <= 0).all() and got["Prediction"].between(0, 1).all()
    raters = set(new[new.anime_id == q].user_id.tolist())
    assert raters and not set(got["user_id"]) & raters and set(got["user_id"]) <= set(model["user_ids"].tolist())
    # no user outside the list and the raters is predicted above the list's last
    from anime_recommendations_amd import ops, weights_io
    U = _cuda(np.asarray(model["U"], np.float32))
    everyone = np.arange(len(model["user_ids"]), dtype=np.int32)
    p_all = ops.predict_pairs(U, folded["rows"], weights_io.model_head(model), everyone, np.full(len(everyone), 7, np.int32)).cpu().numpy()
    rest = ~np.isin(model["user_ids"], list(raters | set(got["user_id"])))
    assert p_all[rest].max() <= got["Prediction"].iloc[-1] + 1e-6
    # a count past the users who can be listed returns them all
    got_all, _ = C.new_anime_audience_frame(model, folded, q, 10 ** 6)
    assert len(got_all) == len(model["user_ids"]) - len(raters)


def test_audience_predictions_are_predict_pairs_bits(trained, folded_12):
    """the Prediction column equals ops.predict_pairs on the same (user row, folded row) pairs bit for bit"""
    from anime_recommendations_amd import components as C, ops, weights_io
    out, model, new, folded = folded_12
    q = int(folded["ids"][7])
    got, _ = C.new_anime_audience_frame(model, folded, q, 20)
    pos = {int(u): i for i, u in enumerate(model["user_ids"])}
    rows = np.array([pos[int(u)] for u in got["user_id"]], np.int32)
    U = _cuda(np.asarray(model["U"], np.float32))
    p = ops.predict_pairs(U, folded["rows"], weights_io.model_head(model), rows, np.full(len(rows), 7, np.int32)).cpu().numpy()
    mine = got["Prediction"].to_numpy().astype(np.float32)
    print("audience predictions against predict_pairs: %d of %d differ, largest distance %.3g"
          % (int((_bits(mine) != _bits(p)).sum()), len(p), np.abs(mine.astype(np.float64) - p).max()))
    assert np.array_equal(_bits(mine), _bits(p))


def test_round_trip_through_a_model_file(trained, folded_12, tmp_path):
    from anime_recommendations_amd import components as C, recs, weights_io
    frame, table, res = trained
    out, model, new, folded = folded_12
    anime_df, syn_df = _loaded(tmp_path, frame)
    ext = recs.append_anime(model, folded)
    path = str(tmp_path / "extended.h5")
    weights_io.save_model(path, ext["U"], ext["A"], ext["head"], ext["user_ids"], ext["anime_ids"], activation="sigmoid",
                          loss="binary_crossentropy")
    back = weights_io.load_model(path)
    assert np.asarray(back["U"]).tobytes() == np.asarray(model["U"], np.float32).tobytes()
    assert np.asarray(back["A"])[:len(model["A"])].tobytes() == np.asarray(model["A"], np.float32).tobytes()
    assert np.array_equal(_bits(np.asarray(back["A"])[len(model["A"]):]), _bits(folded["rows"].cpu().numpy()))
    assert np.asarray(back["anime_ids"]).tolist() == model["anime_ids"].tolist() + folded["ids"].tolist()
    assert back["head"] == pytest.approx(model["head"])
    # similar_anime on the file, for a new anime's name, is new_anime_similar_frame once the other new anime are filtered
    names = dict(zip(anime_df.anime_id, anime_df.Name))
    q = int(folded["ids"][4])
    new_names = {names[int(a)] for a in folded["ids"]}
    served, _ = C.similar_anime_frame(back["A"], back["anime_ids"], anime_df, syn_df, names[q], len(back["anime_ids"]) - 1)
    served = served[~served["Name"].isin(new_names)].reset_index(drop=True)
    mine, _ = C.new_anime_similar_frame(model, folded, anime_df, syn_df, q, len(model["anime_ids"]))
    assert len(mine) == len(served) == int(C.filter_mask(C.metadata_by_index(model["anime_ids"], anime_df, syn_df), anime_df).sum())
    assert served["Name"].tolist() == mine["Name"].tolist()
    assert np.array_equal(_bits(served["Similarity"].to_numpy(np.float32)), _bits(mine["Similarity"].to_numpy(np.float32)))
    # model_recs on the file can now recommend the new anime: to a trained user who has not rated them, asking for every anime
    rated_new = frame[frame.anime_id.isin(folded["ids"])].groupby("user_id").anime_id.nunique()
    user = int(next(u for u in model["user_ids"] if rated_new.get(int(u), 0) < len(folded["ids"])))
    seen = set(frame[frame.user_id == user].anime_id.tolist())
    unseen_new = [int(a) for a in folded["ids"] if int(a) not in seen]
    recs_frame = C.model_recs_frame(back["U"], back["A"], weights_io.model_head(back), back["user_ids"], back["anime_ids"], frame,
                                    anime_df, syn_df, user, len(back["anime_ids"]))
    assert set(unseen_new) <= set(recs_frame["anime_id"].tolist())
    before = C.model_recs_frame(model["U"], model["A"], weights_io.model_head(model), model["user_ids"], model["anime_ids"], frame,
                                anime_df, syn_df, user, len(model["anime_ids"]))
    assert not set(folded["ids"].tolist()) & set(before["anime_id"].tolist())


def test_new_anime_component(trained, tmp_path):
    """the component end to end in a child process: its four outputs, the rows those of recs.fold_in_anime"""
    from anime_recommendations_amd import artifacts, ops, recs, weights_io
    frame, table, res = trained
    out = _most_rated(table, 3, skip=33)                 # some 210 of the 300 users rated each: an audience is left
    model = _without_anime(table, res, out)
    new_ids = np.asarray(table.anime_ids)[out]
    new = frame[frame.anime_id.isin(new_ids)][["user_id", "anime_id", "rating"]].reset_index(drop=True)
    new = pd.concat([new, pd.DataFrame({"user_id": [10 ** 7], "anime_id": [int(new_ids[1])], "rating": [0.5]})])   # no such row
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(tmp_path / "store"))
    prev = os.environ.get("ANIREC_ARTIFACT_DIR")
    os.environ["ANIREC_ARTIFACT_DIR"] = env["ANIREC_ARTIFACT_DIR"]
    try:
        anime, syn = _tables(frame)
        paths = {k: str(tmp_path / k) for k in ("all_anime.csv", "synopses.csv", "new.parquet", "m.h5")}
        anime.to_csv(paths["all_anime.csv"], index=False)
        syn.to_csv(paths["synopses.csv"], index=False)
        new.to_parquet(paths["new.parquet"], index=False)
        weights_io.save_model(paths["m.h5"], model["U"], model["A"], model["head"], model["user_ids"], model["anime_ids"],
                              activation="sigmoid", loss="binary_crossentropy")
        artifacts.log_artifact("all_anime.csv", paths["all_anime.csv"], "raw_data")
        artifacts.log_artifact("synopses.csv", paths["synopses.csv"], "raw_data")
        artifacts.log_artifact("wandb_anime_nn.h5", paths["m.h5"], "h5")
        query = int(new_ids[1])
        flags = dict(main_df="user_stats.parquet:latest", main_df_type="parquet", project_name="anime_recommendations",
                     anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopses_df="synopses.csv:latest",
                     sypnopsis_df_type="raw_data", model="wandb_anime_nn.h5:latest", model_type="h5", a_query_number=10,
                     anime_rec_genres='["Action", "Comedy", None]', types='["TV", "Movie"]', a_rec_type="csv",
                     ID_emb_name="user_embedding", anime_emb_name="anime_embedding", random_anime=False,
                     an_spec_genres=True, spec_types=True, save_sim_anime=True, new_ratings=paths["new.parquet"],
                     fold_steps=40, fold_lr=0.01, audience_number=15, anime_query=query, output_model="extended.h5")
        argv = [sys.executable, os.path.join(ROOT, "new_anime", "new_anime.py")]
        for k, v in flags.items():
            argv += ["--" + k, str(v)]
        r = subprocess.run(argv, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        folded_path = artifacts.use_artifact("folded_anime.npz:latest")
        model_path = artifacts.use_artifact("extended.h5:latest")
    finally:
        if prev is None:
            os.environ.pop("ANIREC_ARTIFACT_DIR", None)
        else:
            os.environ["ANIREC_ARTIFACT_DIR"] = prev
    near = pd.read_csv(tmp_path / ("Anime_ID_%d_similar.csv" % query))
    assert len(near) == 10 and (np.diff(near["Similarity"]) <= 0).all()
    assert near["Type"].isin(["TV", "Movie"]).all() and near["Genres"].str.contains("Action|Comedy").all()
    audience = pd.read_csv(tmp_path / ("Anime_ID_%d_audience.csv" % query))
    assert audience.columns.tolist() == ["user_id", "Prediction"] and len(audience) == 15
    assert not set(audience["user_id"]) & set(new[new.anime_id == query].user_id)
    # folded_anime.npz holds every anime of the file, rows and losses as ops.fold_in_split gives them
    z = np.load(folded_path)
    ids, off, u_idx, rat, dropped = recs.fold_in_anime_csr(new, model["user_ids"], model["anime_ids"])
    assert dropped == 1 and z["ids"].tolist() == ids.tolist() and set(ids.tolist()) == set(new_ids.tolist())
    init = np.asarray(model["A"], np.float32).mean(axis=0, dtype=np.float32)
    rows, ls = ops.fold_in_split(_cuda(np.asarray(model["U"], np.float32)), dict(model["head"], activation="sigmoid"), off, u_idx,
                                 rat, init, lr=0.01, steps=40, l2=1e-4, loss="binary_crossentropy")
    assert np.array_equal(_bits(z["rows"]), _bits(rows.cpu().numpy())) and np.array_equal(_bits(z["loss"]), _bits(ls.cpu().numpy()))
    # and the extended model file carries them at the end of the anime table, the user table untouched
    back = weights_io.load_model(model_path)
    assert np.asarray(back["anime_ids"]).tolist() == model["anime_ids"].tolist() + ids.tolist()
    assert np.array_equal(_bits(np.asarray(back["A"])[-len(ids):]), _bits(z["rows"]))
    assert np.asarray(back["U"]).tobytes() == np.asarray(model["U"], np.float32).tobytes()
