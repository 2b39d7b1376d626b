"""GPU tests of the favourite profiles (anirec_fave_profile), of anirec_user_recs_ex and of the user_prefs /
user_recs components end to end, against the NumPy restatement (tests/prefs_restatement.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import prefs_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand_bits(rng, rows, n, density):
    return R.pack(rng.random((rows, n)) < density)


@pytest.mark.parametrize("n_anime", [1, 31, 32, 33, 549 * 32, 17_560, 131_071])
@pytest.mark.parametrize("n_cat", [1, 31, 32, 33, 64, 128])
def test_fave_profile_equals_restatement(n_anime, n_cat):
    import torch
    from anime_recommendations_amd import recs
    rng = np.random.default_rng(n_anime * 131 + n_cat)
    n_users = 40
    fav = _rand_bits(rng, n_users, n_anime, 0.02 if n_anime > 1000 else 0.3)
    fav[3] = R.pack(np.ones((1, n_anime), bool))[0]            # all-ones row
    fav[4] = 0                                                  # empty row
    cat = _rand_bits(rng, n_anime, n_cat, 0.2)
    cat[: max(1, n_anime // 3), 0] |= 1                         # a category most anime carry
    tf = torch.from_numpy(fav.view(np.int32)).cuda()
    got = recs.fave_profile(tf, cat, n_cat).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (n_users, n_cat)
    np.testing.assert_array_equal(got, R.fave_profile(fav, n_anime, cat, n_cat))
    users = [3, 0, 4, 3, 39, 17, 17, 4]                         # repeats, empty and all-ones rows
    got = recs.fave_profile(tf, cat, n_cat, users=users).cpu().numpy()
    np.testing.assert_array_equal(got, R.fave_profile(fav, n_anime, cat, n_cat, users=users))


def test_fave_profile_out_of_range_user_sets_err_flag():
    import ctypes
    import torch
    from anime_recommendations_amd import _lib, recs
    rng = np.random.default_rng(7)
    fav = _rand_bits(rng, 10, 100, 0.3)
    cat = _rand_bits(rng, 100, 40, 0.3)
    tf = torch.from_numpy(fav.view(np.int32)).cuda()
    with pytest.raises(ValueError, match="out of range"):
        recs.fave_profile(tf, cat, 40, users=[1, 10])
    lib = _lib.load()
    users = torch.tensor([1, -1, 10, 2], dtype=torch.int32).cuda()
    tc = torch.from_numpy(cat.view(np.int32)).cuda()
    counts = torch.full((4, 40), 99, dtype=torch.int32).cuda()
    err = torch.zeros(1, dtype=torch.int32).cuda()
    _lib.check(lib.anirec_fave_profile(_lib.ptr(tf), 10, 100, _lib.ptr(users), 4, _lib.ptr(tc), 40,
                                       _lib.ptr(counts), _lib.ptr(err), ctypes.c_void_p(0)))
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    c = counts.cpu().numpy()
    assert (c[1] == 0).all() and (c[2] == 0).all()
    np.testing.assert_array_equal(c[[0, 3]], R.fave_profile(fav, 100, cat, 40, users=[1, 2]))
    assert lib.anirec_fave_profile(_lib.ptr(tf), 10, 100, None, 9, _lib.ptr(tc), 40, _lib.ptr(counts),
                                   _lib.ptr(err), ctypes.c_void_p(0)) != 0          # users NULL needs n_rows == n_users
    assert lib.anirec_fave_profile(_lib.ptr(tf), 10, 100, None, 10, _lib.ptr(tc), 129, _lib.ptr(counts),
                                   _lib.ptr(err), ctypes.c_void_p(0)) != 0          # n_cat <= 128


def test_fave_profile_full_shape():
    """All users at 350 000 x 17 560 on the favourites of a synthetic rating table: a row sample equals the
    restatement, the column totals equal a NumPy popcount total."""
    import torch
    from anime_recommendations_amd import recs
    n_users, n_anime, n_cat = 350_000, 17_560, 43
    rng = np.random.default_rng(3)
    ww = (n_anime + 31) // 32
    u = np.repeat(np.arange(n_users, dtype=np.int64), 60)           # ~60 favourites per user (repeats collapse)
    a = rng.integers(0, n_anime, len(u))
    fav_np = np.zeros(n_users * ww, np.uint32)
    np.bitwise_or.at(fav_np, u * ww + (a >> 5), np.uint32(1) << (a & 31).astype(np.uint32))
    fav_np = fav_np.reshape(n_users, ww)
    fav = torch.from_numpy(fav_np.view(np.int32)).cuda()
    cat = _rand_bits(rng, n_anime, n_cat, 0.07)
    cat[:, 0] |= (rng.random(n_anime) < 0.6).astype(np.uint32)     # "Action": most anime
    got = recs.fave_profile(fav.contiguous(), cat, n_cat).cpu().numpy()
    rows = rng.choice(n_users, 500, replace=False)
    np.testing.assert_array_equal(got[rows], R.fave_profile(fav_np[rows], n_anime, cat, n_cat))
    per_anime = np.bincount(np.unique(u * n_anime + a) % n_anime, minlength=n_anime)    # popcount total per anime
    want_tot = per_anime @ R.unpack(cat, n_cat).astype(np.int64)
    np.testing.assert_array_equal(got.sum(0, dtype=np.int64), want_tot)


def test_user_recs_ex_equals_user_recs_and_restatement():
    import torch
    from anime_recommendations_amd import recs
    for n_anime, k_sim in ((17_560, 10), (1_000, 40), (70, 63)):
        rng = np.random.default_rng(n_anime + k_sim)
        n_users, nq, n_recs = 300, 64, 10 if n_anime > 100 else 256
        fav = _rand_bits(rng, n_users, n_anime, 0.02 if n_anime > 5000 else 0.2)
        tf = torch.from_numpy(fav.view(np.int32)).cuda()
        q = rng.integers(0, n_users, nq)
        sim = rng.integers(0, n_users, (nq, k_sim))
        sim[::5, -2:] = -1
        a0, c0 = recs.user_recs(tf, n_anime, q, sim, n_recs)
        a1, c1 = recs.user_recs(tf, n_anime, None, sim, n_recs, exclude=fav[q])
        assert torch.equal(a0, a1) and torch.equal(c0, c1)
        excl = _rand_bits(rng, nq, n_anime, 0.1)
        keep = R.pack(rng.random(n_anime) < 0.7)
        a2, c2 = recs.user_recs(tf, n_anime, None, sim, n_recs, exclude=excl, keep=keep)
        a2, c2 = a2.cpu().numpy(), c2.cpu().numpy()
        favs = [set(np.nonzero(r)[0].tolist()) for r in R.unpack(fav, n_anime)]
        ks = set(np.nonzero(R.unpack(keep, n_anime))[0].tolist())
        for i in range(nq):
            ex = set(np.nonzero(R.unpack(excl[i], n_anime))[0].tolist())
            order, counts = R.user_recs(favs, ex, sim[i].tolist(), n_recs, ks)
            assert a2[i][: len(order)].tolist() == order and c2[i][: len(order)].tolist() == counts
            assert (a2[i][len(order):] == -1).all()


# ---------------------------------------------------------------------------------------- end to end
def _run(comp, flags, cwd, env, ok=True):
    argv = [sys.executable, os.path.join(ROOT, comp, comp + ".py")]
    for k, v in flags.items():
        argv += ["--" + k, str(v)]
    r = subprocess.run(argv, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout.decode()[-3000:]
    return r


@pytest.fixture(scope="module")
def flow(tmp_path_factory):
    from anime_recommendations_amd import artifacts, data, weights_io
    work = tmp_path_factory.mktemp("userflow")
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(work / "store"), MPLBACKEND="Agg")
    os.environ["ANIREC_ARTIFACT_DIR"] = env["ANIREC_ARTIFACT_DIR"]
    paths = data.write_synthetic_dataset(str(work / "data"), n_users=300, n_anime=500, n_ratings=40_000, seed=4)
    artifacts.log_artifact("user_stats.parquet", paths["user_stats"], "parquet")
    artifacts.log_artifact("all_anime.csv", paths["all_anime"], "raw_data")
    artifacts.log_artifact("synopses.csv", paths["synopses"], "raw_data")
    df = pd.read_parquet(paths["user_stats"])
    rng = np.random.default_rng(9)
    U = rng.standard_normal((df.user_id.nunique(), 128)).astype(np.float32)
    A = rng.standard_normal((df.anime_id.nunique(), 128)).astype(np.float32)
    head = dict(w=1.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0)
    mp = str(work / "wandb_anime_nn.h5")
    weights_io.save_model(mp, U, A, head, user_ids=df.user_id.unique(), anime_ids=df.anime_id.unique())
    artifacts.log_artifact("wandb_anime_nn.h5", mp, "h5")
    user = int(df.user_id.unique()[7])
    common = dict(project_name="anime_recommendations", model="wandb_anime_nn.h5:latest",
                  main_df="user_stats.parquet:latest", main_df_type="parquet", anime_df="all_anime.csv:latest",
                  anime_df_type="raw_data")
    su = dict(common, model_type="h5", ID_emb_name="user_embedding", anime_emb_name="anime_embedding",
              sim_user_query=user, id_query_number=10, max_ratings=600, sim_random_user=False, num_faves=3,
              TV_only=False, sim_users_fn="similar_users.csv", sim_users_type="csv", ID_fn="user_id.csv",
              ID_type="csv", save_sim_locally=True)
    _run("similar_users", su, str(work), env)
    up = dict(common, prefs_user_query=user, favorite_percentile=80, show_clouds=False,
              genre_fn="favorite_genres.png", source_fn="favorite_sources.png", cloud_width=400, cloud_height=250,
              prefs_csv="user_prefs.csv", interval=100, save_faves=True, flow_user="user_id.csv:latest",
              prefs_from_flow=True, prefs_local_user=False, ID_type="csv", cloud_type="png", fave_art_type="csv")
    _run("user_prefs", up, str(work), env)
    ur = dict(common, model_type="h5", ID_emb_name="user_embedding", anime_emb_name="anime_embedding",
              user_recs_query=user, user_recs_fn="user_recs.csv", save_user_recs=True,
              sypnopses_df="synopses.csv:latest", sypnopsis_df_type="raw_data", user_num_recs=10,
              user_recs_type="csv", flow_ID="user_id.csv:latest", flow_ID_type="csv",
              sim_users_art="similar_users.csv:latest", sim_users_art_type="csv", recs_n_sim_ID=10,
              recs_ID_from_conf=False, ID_rec_genres='["Action", "Comedy", "Drama"]', ID_spec_genres=False,
              prefs_input_fn="user_prefs.csv:latest", prefs_input_type="csv", ID_recs_from_flow=True,
              raise_flow_error=True, ID_recs_faves_fn="recs_faves.csv", ID_recs_faves_type="csv",
              n_flow_sim_IDs=10)
    _run("user_recs", ur, str(work), env)
    return dict(work=work, env=env, paths=paths, user=user, df=df, up=up, ur=ur)


def _fav_sets(df, pct):
    from anime_recommendations_amd.data import encode_ids
    from oracle import recs_oracle
    _, user_ids = encode_ids(df["user_id"].to_numpy())
    _, anime_ids = encode_ids(df["anime_id"].to_numpy())
    from anime_recommendations_amd import components as C
    ui, ai, r = C.rating_indices(df, user_ids, anime_ids)
    _, fav = recs_oracle.favourites(ui, ai, r, len(user_ids), pct)
    return user_ids, anime_ids, fav


def test_user_prefs_flow_outputs(flow, golden_dir):
    from PIL import Image
    from anime_recommendations_amd import artifacts, components as C
    work, user = flow["work"], flow["user"]
    fmt = json.load(open(os.path.join(golden_dir, "user_component_formats.json")))["User_ID_153695_user_prefs.csv"]
    prefs = pd.read_csv(work / ("User_ID_%d_user_prefs.csv" % user))
    assert [("" if c.startswith("Unnamed") else c) for c in prefs.columns] == fmt["columns"]
    user_ids, anime_ids, fav = _fav_sets(flow["df"], 80)
    anime_df = C.load_user_anime_df(flow["paths"]["all_anime"])
    want = C.fave_frame(sorted(fav[C.user_index(user_ids, user)]), anime_ids, anime_df)
    assert prefs.iloc[:, 0].tolist() == want.index.tolist() and prefs["eng_version"].tolist() == want["eng_version"].tolist()
    for fn in ("favorite_genres.png", "favorite_sources.png"):
        assert Image.open(work / ("User_ID_%d_%s" % (user, fn))).size == (400, 250)
    assert artifacts.artifact_metadata("user_prefs.csv")["ID"] == user
    assert artifacts.artifact_metadata("user_prefs.csv")["User_Type"] == "MLflow ID"


def test_user_recs_flow_outputs(flow, golden_dir):
    from PIL import Image
    from anime_recommendations_amd import artifacts, components as C
    work, user = flow["work"], flow["user"]
    fmt = json.load(open(os.path.join(golden_dir, "user_component_formats.json")))["User_ID_153695_user_recs.csv"]
    out = pd.read_csv(work / ("User_ID_%d_user_recs.csv" % user))
    assert out.columns.tolist() == fmt["columns"] and len(out) == fmt["n_rows"]
    assert (np.diff(out["n_user_prefs"]) <= 0).all()
    user_ids, anime_ids, fav = _fav_sets(flow["df"], 80)
    prefs = pd.read_csv(work / ("User_ID_%d_user_prefs.csv" % user))
    sims = pd.read_csv(work / ("User_%d.csv" % user))["similar_users"].tolist()
    anime_df = C.load_user_anime_df(flow["paths"]["all_anime"])
    meta = C.metadata_by_index(anime_ids, anime_df)
    keep = set(np.nonzero(meta["has_meta"].to_numpy())[0].tolist())
    excl = {a for a in keep if meta["eng_version"].iloc[a] in set(prefs["eng_version"])}
    order, counts = R.user_recs(fav, excl, [C.user_index(user_ids, s) for s in sims], 10, keep)
    assert out["anime_id"].tolist() == np.asarray(anime_ids)[order].tolist()
    assert out["n_user_prefs"].tolist() == counts
    assert not set(out["Name"]) & set(prefs["eng_version"])
    for kind in ("genres", "sources"):
        assert Image.open(work / ("User_ID_%d_recs_favorite_%s.png" % (user, kind))).size == (600, 350)
    assert os.path.exists(work / ("User_ID_%d_recs_faves.csv" % user))
    m = artifacts.artifact_metadata("user_recs.csv")
    assert m["Queried user"] == user and m["Flow ID used"] is True


def test_user_recs_genre_groups_and_other_paths(flow):
    from anime_recommendations_amd import components as C
    work, env, user = flow["work"], flow["env"], flow["user"]
    ur = dict(flow["ur"], ID_spec_genres=True, user_recs_fn="user_recs_g.csv", user_num_recs=40)
    _run("user_recs", ur, str(work), env)
    out = pd.read_csv(work / ("User_ID_%d_user_recs_g.csv" % user))
    wanted = C.clean(["Action", "Comedy", "Drama"])
    grp = [next(i for i, g in enumerate(wanted) if g in str(x).lower().replace(" ", "")) for x in out["Genres"]]
    assert grp == sorted(grp) and len(out) > 0
    for g in set(grp):           # n_user_prefs non-increasing except across genre groups
        c = [n for n, x in zip(out["n_user_prefs"], grp) if x == g]
        assert c == sorted(c, reverse=True)
    # non-flow path (config user, similar users by cosine top-k on the model's user table) and a random user
    nf = dict(flow["ur"], ID_recs_from_flow=False, recs_ID_from_conf=True, user_recs_fn="user_recs_nf.csv")
    _run("user_recs", nf, str(work), env)
    assert len(pd.read_csv(work / ("User_ID_%d_user_recs_nf.csv" % user))) == 10
    rnd = dict(flow["ur"], ID_recs_from_flow=False, recs_ID_from_conf=False, user_recs_fn="user_recs_rnd.csv")
    _run("user_recs", rnd, str(work), env)
    assert any(f.endswith("_user_recs_rnd.csv") for f in os.listdir(work))
    rp = dict(flow["up"], prefs_from_flow=False, prefs_local_user=False, prefs_csv="prefs_rnd.csv")
    _run("user_prefs", rp, str(work), env)
    assert any(f.endswith("_prefs_rnd.csv") for f in os.listdir(work))


def test_user_recs_flow_mismatch(flow):
    work, env, user = flow["work"], flow["env"], flow["user"]
    from anime_recommendations_amd import artifacts
    other = int(flow["df"].user_id.unique()[9])
    p = work / "other_id.csv"
    pd.DataFrame([other], columns=["User_ID"]).to_csv(p, index=False)
    artifacts.log_artifact("other_id.csv", str(p), "csv", metadata={"Queried user": other})
    bad = dict(flow["ur"], flow_ID="other_id.csv:latest", user_recs_fn="user_recs_bad.csv")
    r = _run("user_recs", dict(bad, raise_flow_error=True), str(work), env, ok=False)
    assert r.returncode != 0
    r = _run("user_recs", dict(bad, raise_flow_error=False), str(work), env, ok=False)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert not any(f.endswith("_user_recs_bad.csv") for f in os.listdir(work))
