"""GPU half of the similar_anime / model_recs / get_df parity against the reference's own function bodies
(tests/golden/ref_fn/recs.*, tests/golden/make_recs_fixtures.py): components.similar_anime_frame,
components.model_recs_frame and ingest.encode_frame on each fixture input, at counts 10 and 127 (the top-k kernels)
and 129 and every row (the *_topk_large kernels), and the two command-line components once each.

Row counts, columns, every non-score column and the index / shuffle columns are exact; similarities are within 2e-6 of
the fixture's fp64 cosine and predictions within 1e-5 of the float64 model; order as in recs_fixture.check_ranked."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import recs_fixture as RF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = RF.load()
SA, MR = REC["similar_anime"], REC["model_recs"]
ANIME_IDS = REC["npz"]["main_index_to_anime"]
FLAGS = REC["flags"]


def _frames(drop=()):
    from anime_recommendations_amd import components as C
    a = C.load_anime_df(RF.csv(REC, "anime_csv"))
    return a[~a.anime_id.isin(list(drop))], C.load_synopses(RF.csv(REC, "synopses_csv"))


def _check_columns(part, frame, keys, case):
    assert list(frame.columns) == REC[part]["columns"]
    for i, k in enumerate(keys):
        want = RF.expected_columns(REC, part, k)
        for col in frame.columns:
            if col in ("Similarity", "Prediction") or col not in want:
                continue
            assert RF.same_value(frame[col].iloc[i], want[col]), (part, k, col, frame[col].iloc[i], want[col])


def _similar_anime(case, anime_df, syn_df):
    from anime_recommendations_amd import components as C
    return C.similar_anime_frame(REC["npz"]["A"], ANIME_IDS, anime_df, syn_df, case["query"], case["count"],
                                 types=C.literal(FLAGS["SA_TYPES"]) if case["spec_types"] else None,
                                 genres=C.literal(FLAGS["SA_GENRES"]) if case["spec_genres"] else None)


def _sa_keys(frame, anime_df):
    by_name = dict(zip(anime_df["Name"], anime_df["anime_id"]))
    return [int(by_name[n]) for n in frame["Name"]]


@pytest.mark.parametrize("qkey", ["exact", "fallback", "cleaned_name_first"])
def test_similar_anime_frame_equals_anime_recs(qkey):
    anime_df, syn_df = _frames()
    idx_of = {int(a): i for i, a in enumerate(ANIME_IDS)}
    for c in (c for c in SA["cases"] if c["query_key"] == qkey):
        frame, fn = _similar_anime(c, anime_df, syn_df)
        assert fn == c["filename"]
        full = RF.full_case(SA["cases"], c, ("query_key", "spec_types", "spec_genres"))
        keys = _sa_keys(frame, anime_df)
        RF.check_ranked(keys, frame["Similarity"].to_numpy(), c["anime_id"], full["anime_id"], full["cos64"],
                        RF.SIM_BAR, got_index=[idx_of[k] for k in keys])
        _check_columns("similar_anime", frame, keys, c)


def test_similar_anime_drops_an_anime_without_metadata():
    """The reference raises IndexError when an embedded anime has no all_anime.csv row (recorded in the fixture);
    the build drops that row: its list is the reference's every-row list without it."""
    dev = REC["deviations"]["similar_anime_no_metadata"]
    assert dev["reference_error"] == "IndexError"
    gone = dev["anime_id"]
    anime_df, syn_df = _frames([gone])
    idx_of = {int(a): i for i, a in enumerate(ANIME_IDS)}
    for c in SA["cases"]:
        if c["query_key"] != "exact" or c["spec_types"] or c["spec_genres"] or c["count"] not in (10, RF.ALL):
            continue
        full = RF.full_case(SA["cases"], c, ("query_key", "spec_types", "spec_genres"))
        assert gone in full["anime_id"]
        keep = [i for i, a in enumerate(full["anime_id"]) if a != gone]
        f_ids, f_cos = [full["anime_id"][i] for i in keep], [full["cos64"][i] for i in keep]
        frame, _ = _similar_anime(c, anime_df, syn_df)
        keys = _sa_keys(frame, anime_df)
        RF.check_ranked(keys, frame["Similarity"].to_numpy(), f_ids[:c["count"]], f_ids, f_cos, RF.SIM_BAR,
                        got_index=[idx_of[k] for k in keys])


def _model_recs(case, anime_df, syn_df, user_ids, df):
    from anime_recommendations_amd import components as C
    z = REC["npz"]
    return C.model_recs_frame(z["U"], z["A"], dict(MR["heads"][case["activation"]], activation=case["activation"]), user_ids, ANIME_IDS,
                              df, anime_df, syn_df, case["user"], case["n_recs"],
                              types=C.literal(FLAGS["MR_TYPES"]) if case["spec_types"] else None,
                              genres=C.literal(FLAGS["MR_GENRES"]) if case["spec_genres"] else None)


@pytest.mark.parametrize("act", ["sigmoid", "relu"])
def test_model_recs_frame_equals_recommendations(act):
    """Cases the reference cannot run (no Type filter: KeyError; a Genre filter: AttributeError) are held to the
    frames the generator pinned from the reference's own bodies (make_recs_fixtures.pinned_model_recs)."""
    from anime_recommendations_amd import components as C
    df = RF.ratings(REC)
    user_ids, aids = C.index_tables({}, df)
    assert np.array_equal(aids, ANIME_IDS)
    anime_df, syn_df = _frames(MR["no_metadata"])
    idx_of = {int(a): i for i, a in enumerate(ANIME_IDS)}
    for c in (c for c in MR["cases"] if c["activation"] == act):
        frame = _model_recs(c, anime_df, syn_df, user_ids, df)
        full = RF.full_case(MR["cases"], c, ("user", "activation", "spec_types", "spec_genres"))
        keys = frame["anime_id"].astype(np.int64).tolist()
        RF.check_ranked(keys, frame["Prediction"].to_numpy(), c["anime_id"], full["anime_id"], full["prediction"],
                        RF.PRED_BAR, got_index=[idx_of[k] for k in keys])
        _check_columns("model_recs", frame, keys, c)


def test_gpu_encode_frame_equals_get_df_and_main_df_by_anime():
    from anime_recommendations_amd import data, ingest
    z = REC["npz"]
    for prefix, mr in (("ratings", None), ("ratings", 400), ("minr", None), ("minr", 400)):
        df = RF.ratings(REC, prefix)
        t = ingest.encode_frame(df, min_ratings=mr)
        h = data.encode_frame(df, min_ratings=mr)
        if prefix == "ratings":
            want = ("get_df_user", "get_df_anime") if mr is None else ("main_user", "main_anime")
            assert np.array_equal(t.user, z[want[0]]) and np.array_equal(t.anime, z[want[1]])
            rating = z["get_df_rating"] if mr is None else z["main_rating"]
            assert np.array_equal(np.asarray(t.rating, np.float64).view(np.uint64), rating.view(np.uint64))
            assert np.array_equal(t.anime_ids, ANIME_IDS)
        else:
            want = z["minr_get_df_anime"] if mr is None else z["minr_main_anime"]
            assert np.array_equal(t.anime, want)
            if mr:
                assert np.array_equal(t.user, z["minr_main_user"])
                assert np.array_equal(t.anime_ids, z["minr_main_index_to_anime"])
        for f in ("user", "anime", "user_ids", "anime_ids"):
            assert np.array_equal(getattr(t, f), getattr(h, f)), f
    assert np.array_equal(data.shuffle_order(len(RF.ratings(REC))), z["get_df_index"])


# ---------------------------------------------------------------------------------------- command line
def _run(comp, flags, cwd, env):
    argv = [sys.executable, os.path.join(ROOT, comp, comp + ".py")]
    for k, v in flags.items():
        argv += ["--" + k, str(v)]
    r = subprocess.run(argv, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_command_line_components_write_the_frames(tmp_path):
    from anime_recommendations_amd import artifacts, components as C, weights_io
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(tmp_path / "store"))
    old = os.environ.get("ANIREC_ARTIFACT_DIR")
    os.environ["ANIREC_ARTIFACT_DIR"] = env["ANIREC_ARTIFACT_DIR"]
    try:
        z, df = REC["npz"], RF.ratings(REC)
        user_ids, _ = C.index_tables({}, df)
        pq = str(tmp_path / "user_stats.parquet")
        df.to_parquet(pq, index=False)
        anime_csv, syn_csv = str(tmp_path / "all_anime.csv"), str(tmp_path / "synopses.csv")
        (tmp_path / "all_anime.csv").write_bytes(z["anime_csv"].tobytes())
        (tmp_path / "synopses.csv").write_bytes(z["synopses_csv"].tobytes())
        raw = pd.read_csv(anime_csv)
        mr_csv = str(tmp_path / "all_anime_mr.csv")
        raw[~raw.MAL_ID.isin(MR["no_metadata"])].to_csv(mr_csv, index=False)
        c_sa = next(c for c in SA["cases"] if c["query_key"] == "fallback" and c["spec_types"] and c["spec_genres"]
                    and c["count"] == 10)
        c_mr = next(c for c in MR["cases"] if c["activation"] == "relu" and c["spec_types"] and not c["spec_genres"]
                    and c["n_recs"] == 129)
        mp = str(tmp_path / "wandb_anime_nn.h5")
        weights_io.save_model(mp, z["U"], z["A"], dict(MR["heads"]["relu"], activation="relu"), user_ids=user_ids,
                              anime_ids=ANIME_IDS)
        for name, path, kind in (("user_stats.parquet", pq, "parquet"), ("all_anime.csv", anime_csv, "raw_data"),
                                 ("all_anime_mr.csv", mr_csv, "raw_data"),
                                 ("synopses.csv", syn_csv, "raw_data"), ("wandb_anime_nn.h5", mp, "h5")):
            artifacts.log_artifact(name, path, kind)
        common = dict(project_name="anime_recommendations", model="wandb_anime_nn.h5:latest", model_type="h5",
                      main_df="user_stats.parquet:latest", main_df_type="parquet", anime_df_type="raw_data",
                      sypnopsis_df_type="raw_data")
        sa = dict(common, anime_df="all_anime.csv:latest", sypnopses_df="synopses.csv:latest",
                  anime_query=c_sa["query"], a_query_number=c_sa["count"], random_anime=False,
                  anime_rec_genres=FLAGS["SA_GENRES"], an_spec_genres=True, types=FLAGS["SA_TYPES"], spec_types=True,
                  a_rec_type="csv", save_sim_anime=True, ID_emb_name="user_embedding",
                  anime_emb_name="anime_embedding")
        _run("similar_anime", sa, str(tmp_path), env)
        anime_df, syn_df = _frames()
        want, fn = _similar_anime(c_sa, anime_df, syn_df)
        assert (tmp_path / fn).read_text() == want.to_csv(index=False)
        mr = dict(common, anime_df="all_anime_mr.csv:latest", sypnopsis_df="synopses.csv:latest",
                  model_user_query=c_mr["user"], model_recs_fn="model_recs.csv", model_num_recs=c_mr["n_recs"],
                  anime_types=FLAGS["MR_TYPES"], model_genres=FLAGS["MR_GENRES"], model_recs_type="csv",
                  flow_ID="user_id.csv:latest", flow_ID_type="csv", random_user=False, save_model_recs=True,
                  specify_types=True, specify_genres=False, model_ID_flow=False, model_ID_conf=True)
        _run("model_recs", mr, str(tmp_path), env)
        anime_df, syn_df = _frames(MR["no_metadata"])
        want = _model_recs(c_mr, anime_df, syn_df, user_ids, df)
        got = (tmp_path / ("User_ID_%d_model_recs.csv" % c_mr["user"])).read_text()
        assert got == want.to_csv(index=False)
        assert len(want) == len(c_mr["anime_id"]) and len(want) > 0
    finally:
        if old is None:
            os.environ.pop("ANIREC_ARTIFACT_DIR", None)
        else:
            os.environ["ANIREC_ARTIFACT_DIR"] = old
