"""CPU half of the similar_anime / model_recs / get_df parity against the reference's own function bodies
(tests/golden/ref_fn/recs.*, tests/golden/make_recs_fixtures.py): the host pieces of components.py and data.py — the
metadata table, the query lookup, the Type / Genre / unwatched masks, the count clamp, the id encodings and the
shuffle — and the oracle's top-k on the fixture's own scores."""
import numpy as np
import pandas as pd
import pytest

import recs_fixture as RF
from anime_recommendations_amd import components as C, data
from oracle import anirec_oracle as orc

REC = RF.load()
SA, MR = REC["similar_anime"], REC["model_recs"]
ANIME_IDS = REC["npz"]["main_index_to_anime"]
FLAGS = REC["flags"]


def _anime_df(drop=()):
    a = C.load_anime_df(RF.csv(REC, "anime_csv"))
    return a[~a.anime_id.isin(list(drop))]


def _meta(drop=()):
    return C.metadata_by_index(ANIME_IDS, _anime_df(drop), C.load_synopses(RF.csv(REC, "synopses_csv")))


def _sa_keep(case, meta):
    return C.filter_mask(meta, _anime_df(), C.literal(FLAGS["SA_TYPES"]) if case["spec_types"] else None,
                         C.literal(FLAGS["SA_GENRES"]) if case["spec_genres"] else None)


def _mr_keep(case, meta, df):
    return C.unwatched_mask(df, ANIME_IDS, case["user"]) & C.filter_mask(
        meta, _anime_df(MR["no_metadata"]), C.literal(FLAGS["MR_TYPES"]) if case["spec_types"] else None,
        C.literal(FLAGS["MR_GENRES"]) if case["spec_genres"] else None)


def test_fixture_covers_the_edges():
    counts = {c["count"] for c in SA["cases"]} | {c["n_recs"] for c in MR["cases"]}
    assert {10, 127, 129, RF.ALL} <= counts
    assert {c["query_key"] for c in SA["cases"]} == {"exact", "fallback", "cleaned_name_first"}
    assert {c["activation"] for c in MR["cases"]} == {"sigmoid", "relu"}
    assert any(len(c["anime_id"]) < c["count"] for c in SA["cases"])        # a filter leaves fewer rows
    assert any(len(c["anime_id"]) < c["n_recs"] for c in MR["cases"])
    assert any(len(c["anime_id"]) > 128 for c in SA["cases"]) and any(len(c["anime_id"]) > 128 for c in MR["cases"])
    assert not REC["npz"]["A"][REC["zero_row"]].any()                         # a zero row: NaN similarities
    full = next(c for c in SA["cases"] if c["query_key"] == "exact" and c["count"] == RF.ALL
                and not c["spec_types"] and not c["spec_genres"])
    assert RF.is_null(full["cos64"][-1])                                       # NaN similarity listed, last
    cos = full["cos64"]
    assert cos[9] == cos[10] and cos[126] == cos[127] and cos[128] == cos[129]   # exact ties straddle the cuts
    relu = [c for c in MR["cases"] if c["activation"] == "relu" and c["n_recs"] == RF.ALL]
    assert all(c["prediction"].count(0.0) > 1 for c in relu)                   # the flat region ties
    assert SA["rows"]["data"] and MR["rows"]["data"]
    dev = REC["deviations"]
    assert dev["similar_anime_no_metadata"]["reference_error"] == "IndexError"
    assert dev["model_recs_specify_types_false"]["reference_error"] == "KeyError"
    assert dev["model_recs_specify_genres_true"]["reference_error"] == "AttributeError"
    assert dev["main_df_by_anime_min_ratings"]["encodings_agree"] is False
    assert dev["model_recs_shuffled_encoding"]["anime_orders_agree"] is False


def test_metadata_by_index_equals_the_reference_rows():
    for part, drop in (("similar_anime", ()), ("model_recs", MR["no_metadata"])):
        meta = _meta(drop).set_index("anime_id")
        rows = REC[part]["rows"]
        for key, vals in rows["data"].items():
            m = meta.loc[int(key)]
            assert m["has_meta"]
            for col, v in zip(rows["columns"], vals):
                if col == "anime_id":
                    continue
                assert RF.same_value(m[RF.META_COL.get(col, col)], v), (part, key, col, m[RF.META_COL.get(col, col)], v)
    meta = _meta(MR["no_metadata"]).set_index("anime_id")
    assert not meta.loc[MR["no_metadata"], "has_meta"].any()


def test_find_anime_id_resolves_each_query_like_the_reference():
    adf = _anime_df()
    for c in SA["cases"]:
        assert C.find_anime_id(c["query"], adf) == c["query_id"], c["query_key"]
        assert C.clean(c["query"]) + ".csv" == c["filename"]


def test_type_and_genre_masks_keep_the_reference_rows():
    meta = _meta()
    for c in SA["cases"]:
        if c["count"] != RF.ALL:
            continue
        keep = _sa_keep(c, meta)
        keep[ANIME_IDS == c["query_id"]] = False
        assert set(ANIME_IDS[keep].tolist()) == set(c["anime_id"]), (c["query_key"], c["spec_types"], c["spec_genres"])


def test_unwatched_mask_keeps_the_reference_rows():
    df, meta = RF.ratings(REC), _meta(MR["no_metadata"])
    for c in MR["cases"]:
        if c["n_recs"] != RF.ALL:
            continue
        assert set(ANIME_IDS[_mr_keep(c, meta, df)].tolist()) == set(c["anime_id"]), (c["user"], c["activation"])


def test_count_clamp_gives_the_reference_row_counts():
    meta, df = _meta(), RF.ratings(REC)
    for c in SA["cases"]:
        keep = _sa_keep(c, meta)
        n_keep = int(keep.sum()) - int(keep[ANIME_IDS == c["query_id"]].any())
        k = C._topk_count(c["count"], "a_query_number", len(ANIME_IDS) - 1)
        assert len(c["anime_id"]) == min(k, n_keep), (c["query_key"], c["count"])
    meta = _meta(MR["no_metadata"])
    for c in MR["cases"]:
        k = C._topk_count(c["n_recs"], "model_num_recs", len(ANIME_IDS))
        assert len(c["anime_id"]) == min(k, int(_mr_keep(c, meta, df).sum())), (c["user"], c["n_recs"])
    for bad in (0, -3):
        with pytest.raises(ValueError):
            C._topk_count(bad, "a_query_number", 10)


def test_check_types_accepts_the_flags_and_refuses_others():
    assert C.check_types(C.literal(FLAGS["SA_TYPES"])) == ["Movie", "Special", "ONA"]
    assert C.check_types(C.literal(FLAGS["MR_TYPES"])) == ["TV", "Movie"]
    with pytest.raises(ValueError):
        C.check_types(["TV", "Film"])


def test_host_encode_frame_equals_get_df_and_main_df_by_anime():
    z, df = REC["npz"], RF.ratings(REC)
    t = data.encode_frame(df)
    assert np.array_equal(data.shuffle_order(len(df)), z["get_df_index"])
    assert np.array_equal(t.user, z["get_df_user"]) and np.array_equal(t.anime, z["get_df_anime"])
    assert np.array_equal(t.rating.view(np.uint64), z["get_df_rating"].view(np.uint64))
    assert (t.n_users, t.n_anime) == (REC["get_df"]["n_users"], REC["get_df"]["n_anime"])
    m = data.encode_frame(df, min_ratings=400)
    assert np.array_equal(m.user, z["main_user"]) and np.array_equal(m.anime, z["main_anime"])
    assert np.array_equal(m.rating.view(np.uint64), z["main_rating"].view(np.uint64))
    assert np.array_equal(m.anime_ids, z["main_index_to_anime"])
    assert np.array_equal(df.index.to_numpy()[data.shuffle_order(len(df))], z["main_index"])
    _, aids = C.index_tables({}, df, min_ratings=400)
    assert np.array_equal(aids, z["main_index_to_anime"])


def test_min_ratings_deviation_is_pinned():
    """main_df_by_anime drops users below 400 ratings before it encodes; get_df does not.  The component takes the
    anime table from the model file (get_df's encoding, the rows the model was trained on) and rebuilds
    main_df_by_anime's only for a model file without one."""
    z, df = REC["npz"], RF.ratings(REC, "minr")
    g = data.encode_frame(df)
    assert np.array_equal(g.anime, z["minr_get_df_anime"])
    assert np.array_equal(data.shuffle_order(len(df)), z["minr_get_df_index"])
    m = data.encode_frame(df, min_ratings=400)
    assert np.array_equal(m.anime, z["minr_main_anime"]) and np.array_equal(m.user, z["minr_main_user"])
    _, aids = C.index_tables({}, df, min_ratings=400)
    assert np.array_equal(aids, z["minr_main_index_to_anime"])
    assert not np.array_equal(g.anime_ids[:len(aids)], aids)
    _, own = C.index_tables({"user_ids": g.user_ids, "anime_ids": g.anime_ids}, df, min_ratings=400)
    assert np.array_equal(own, g.anime_ids)


def test_load_anime_df_equals_get_anime_df():
    want = REC["get_anime_df"]
    a = C.load_anime_df(RF.csv(REC, "anime_csv"))
    assert list(a.columns) == want["columns"]
    assert dict(zip(a.anime_id, a.eng_version)) == dict(zip(want["anime_id"], want["eng_version"]))
    # Score order exact; among equal Scores (the reference's quicksort leaves their order open) as sets
    got = list(zip([None if RF.is_null(s) else s for s in a["Score"]], a.anime_id))
    wnt = list(zip(want["Score"], want["anime_id"]))
    assert [s for s, _ in got] == [s for s, _ in wnt]
    runs = pd.Series([s for s, _ in wnt]).fillna("NaN").ne(pd.Series([s for s, _ in wnt]).fillna("NaN").shift()).cumsum()
    for r in runs.unique():
        sel = np.nonzero((runs == r).to_numpy())[0]
        assert {got[i][1] for i in sel} == {wnt[i][1] for i in sel}


@pytest.mark.parametrize("part", ["similar_anime", "model_recs"])
def test_oracle_topk_on_the_fixture_scores_gives_the_reference_rows(part):
    """orc.topk_desc (the build's defined ranking: desc, ties by index, NaN last) on the fixture's own fp64 scores,
    rounded to fp32, over the rows each setting keeps."""
    cases = REC[part]["cases"]
    idx_of = {int(a): i for i, a in enumerate(ANIME_IDS)}
    keys = ("query_key", "spec_types", "spec_genres") if part == "similar_anime" else \
        ("user", "activation", "spec_types", "spec_genres")
    score = "cos64" if part == "similar_anime" else "prediction"
    bar = RF.SIM_BAR if part == "similar_anime" else RF.PRED_BAR
    for c in cases:
        full = RF.full_case(cases, c, keys)
        s = np.full(len(ANIME_IDS), np.nan, np.float64)
        keep = np.zeros(len(ANIME_IDS), bool)
        for a, v in zip(full["anime_id"], full[score]):
            s[idx_of[a]] = np.nan if v is None else v
            keep[idx_of[a]] = True
        k = c["count"] if part == "similar_anime" else c["n_recs"]
        sel, sc = orc.topk_desc(s.astype(np.float32), min(k, len(ANIME_IDS)), mask=keep)
        RF.check_ranked(ANIME_IDS[sel], sc, c["anime_id"], full["anime_id"], full[score], bar, got_index=sel)
