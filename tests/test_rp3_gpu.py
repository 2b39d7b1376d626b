"""GPU tests of the RP3beta graph baseline (anirec_wcooc_scores; ops.wcooc_scores; recs.rp3_*; the rp3_recs component,
evaluate --baseline rp3 and rp3 as a hybrid_recs member).

Yardstick: the NumPy restatement (tests/rp3_restatement.py).  Every sum is one of integers and every weight a fixed chain
of correctly rounded fp64 operations, so the sums, the excl words and the weights are compared bit for bit.

Shapes: users on both sides of a word, of one MFMA k-step (64) and of one staged chunk (from the size query), with
garbage in the bits past n_users; items on both sides of an MFMA tile (16) and of a workgroup tile (64); 1, 63 and 65
queries, a shuffled draw with repeats; weights that are all 1 (crossed with the popcount kernel), on both sides of the
limb carry, and distinct per user under row and column scales that differ (a transposed write or a misaligned k map
cannot hide); 16 items x 2^24 users with every bit set and the largest weight, for the int32 accumulators."""
import numpy as np
import pytest

import cooc_restatement as CR
import ease_cases as EC
import poison
import recs_fixture as RF
import rp3_cases as RC
import rp3_restatement as R
from component_cli import load_component
from test_cooc_gpu import fixture_store  # noqa: F401  (the recs fixture as an artifact store)

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
WEIGHTS = ("ones", "limbs", "distinct")


def _cuda(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _u32(x):
    return np.ascontiguousarray(_np(x)).view(np.uint32)


def _chunk_users():
    from anime_recommendations_amd import _lib
    return 32 * int(_lib.load().anirec_wcooc_chunk_words())


def _users(case):
    c = _chunk_users()
    return {"chunk-1": c - 1, "chunk": c, "chunk+1": c + 1, "2chunk+4": 2 * c + 4}.get(case, case)


def _check(n_items, n_users, nq, kinds=WEIGHTS, seed=0):
    from anime_recommendations_amd import ops
    bits, B = RC.bits_case(n_items, n_users, seed)
    q = RC.queries(n_items, nq, seed)
    row, col = RC.scales(n_items)
    dbits = _cuda(bits.view(np.int32))
    for kind in kinds:
        uq = RC.user_weights(kind, n_users, seed)
        rs, cs = (None, None) if kind == "ones" else (row, col)
        want_w, want_s, want_ex, err = R.wcooc_scores(bits, n_users, uq, q, rs, cs)
        assert err == 0
        w, s, ex = ops.wcooc_scores(dbits, n_users, uq, q, rs, cs, sums=True, excl=True)
        what = (n_items, n_users, nq, kind)
        assert np.array_equal(_np(s), want_s), what
        assert np.array_equal(_u32(ex), want_ex), what
        assert np.array_equal(_u32(w), _u32(want_w)), what
        if kind == "ones":                                    # the popcount kernel on the same bits
            cnt = ops.cooc_scores(dbits, n_users, q, count=True)[1]
            assert np.array_equal(_np(cnt).astype(np.int64), _np(s)), what


# ---- the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_users", [1, 31, 32, 33, 63, 64, 65, "chunk-1", "chunk", "chunk+1", "2chunk+4"])
def test_sums_weights_and_excl_equal_the_restatement_at_the_user_edges(n_users):
    _check(65, _users(n_users), 63)


@pytest.mark.parametrize("n_items", [1, 15, 16, 17, 63, 64, 65, 130])
def test_sums_weights_and_excl_equal_the_restatement_at_the_item_edges(n_items):
    _check(n_items, 65, min(63, max(1, n_items - 1)))
    _check(n_items, _users("chunk+1"), 1, kinds=("distinct",), seed=1)


@pytest.mark.parametrize("nq", [1, 63, 65])
def test_sums_weights_and_excl_equal_the_restatement_at_the_query_edges(nq):
    _check(130, 100, nq)
    q = RC.queries(130, nq)
    assert nq == 1 or len(set(q.tolist())) < nq               # the draw holds a repeat


def test_the_int32_accumulators_hold_the_largest_sum():
    """16 items x 2^24 users, every bit set, q = 16383: each limb's accumulator ends at 127 * 2^24 < 2^31"""
    import torch
    from anime_recommendations_amd import ops
    n, n_users = 16, 1 << 24
    bits = torch.full((n, n_users // 32), -1, dtype=torch.int32, device="cuda")         # 32 MB
    uq = torch.full((n_users,), RC.MAX_Q, dtype=torch.int32, device="cuda")
    q = np.random.default_rng(0).permutation(n).astype(np.int32)
    w, s, ex = ops.wcooc_scores(bits, n_users, uq, q, sums=True, excl=True)
    assert bool((s == RC.MAX_Q * n_users).all())
    assert np.array_equal(_u32(ex)[:, 0], np.uint32(1) << q.astype(np.uint32))           # only the item itself
    assert bool((w == float(np.float32(np.float64(RC.MAX_Q * n_users)))).all())


def test_bad_queries_and_weights_raise_the_flag_and_spare_the_rest():
    from anime_recommendations_amd import ops
    n_items, n_users = 65, 200
    bits, _ = RC.bits_case(n_items, n_users)
    dbits = _cuda(bits.view(np.int32))
    row, col = RC.scales(n_items)
    uq = RC.user_weights("limbs", n_users)
    q = RC.queries(n_items, 65)
    clean = ops.wcooc_scores(dbits, n_users, uq, q, row, col, sums=True, excl=True)
    q2 = q.copy()
    q2[3], q2[64] = -1, n_items
    want = R.wcooc_scores(bits, n_users, uq, q2, row, col)
    assert want[3] == 1
    w, s, ex, flag = ops.wcooc_scores(dbits, n_users, uq, q2, row, col, sums=True, excl=True, check=False)
    assert int(flag.item()) == 1
    assert np.array_equal(_u32(w), _u32(want[0])) and np.array_equal(_np(s), want[1]) and np.array_equal(_u32(ex), want[2])
    assert (_u32(w)[[3, 64]] == NAN_BITS).all() and (_np(s)[[3, 64]] == -1).all()
    others = [t for t in range(65) if t not in (3, 64)]
    for got, ref in zip((w, s, ex), clean):
        assert np.array_equal(_np(got)[others], _np(ref)[others])
    with pytest.raises(ValueError, match="out of range"):
        ops.wcooc_scores(dbits, n_users, uq, q2)
    uq2 = uq.copy()
    uq2[5], uq2[150] = -1, RC.MAX_Q + 1
    want = R.wcooc_scores(bits, n_users, uq2, q, row, col)
    assert want[3] == 1
    w, s, ex, flag = ops.wcooc_scores(dbits, n_users, uq2, q, row, col, sums=True, excl=True, check=False)
    assert int(flag.item()) == 1
    assert np.array_equal(_u32(w), _u32(want[0])) and np.array_equal(_np(s), want[1]) and np.array_equal(_u32(ex), want[2])
    uq3 = uq.copy()
    uq3[[5, 150]] = 0                                         # "counts as 0"
    zeroed = ops.wcooc_scores(dbits, n_users, uq3, q, row, col, sums=True)
    assert np.array_equal(_np(s), _np(zeroed[1])) and np.array_equal(_u32(w), _u32(zeroed[0]))
    with pytest.raises(ValueError, match="user weight"):
        ops.wcooc_scores(dbits, n_users, uq2, q)
    assert int(ops.wcooc_scores(dbits, n_users, uq, q, check=False)[3].item()) == 0     # the flag is cleared by a call
    assert ops.wcooc_scores(dbits, n_users, uq, [])[0].shape == (0, n_items)


def test_a_row_does_not_depend_on_the_call_the_workspace_or_the_optional_outputs():
    import torch
    from anime_recommendations_amd import ops
    n_items, n_users = 130, _users("chunk+1")
    bits, _ = RC.bits_case(n_items, n_users, 2)
    dbits = _cuda(bits.view(np.int32))
    row, col = RC.scales(n_items)
    uq = RC.user_weights("distinct", n_users, 2)
    q = RC.queries(n_items, 65, 2)
    w, s, ex = ops.wcooc_scores(dbits, n_users, uq, q, row, col, sums=True, excl=True)
    for t in (0, 17, 64):                                     # a query alone is its row among 65
        w1, s1, ex1 = ops.wcooc_scores(dbits, n_users, uq, q[t:t + 1], row, col, sums=True, excl=True)
        assert np.array_equal(_u32(w1)[0], _u32(w)[t]) and torch.equal(s1[0], s[t]) and torch.equal(ex1[0], ex[t])
    again = ops.wcooc_scores(dbits, n_users, uq, q, row, col, sums=True, excl=True)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(again, (w, s, ex)))
    for byte in poison.ORDER:                                 # the workspace and every output start dirty
        log = []
        with poison.poisoned(byte, log):
            dirty = ops.wcooc_scores(dbits, n_users, uq, q, row, col, sums=True, excl=True)
        assert len(log) >= 4                                  # three outputs and the workspace at the least
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(dirty, (w, s, ex))), hex(byte)
    for sums, excl in ((False, False), (True, False), (False, True)):
        got = ops.wcooc_scores(dbits, n_users, uq, q, row, col, sums=sums, excl=excl)
        assert np.array_equal(_u32(got[0]), _u32(w))
        assert (got[1] is None) == (not sums) and (got[2] is None) == (not excl)
        assert got[1] is None or torch.equal(got[1], s)
        assert got[2] is None or torch.equal(got[2], ex)


# ---- the recs layer, on the planted blocks ----------------------------------------------------------------------------
def _planted_fit(neighbours, alpha=1.0, beta=0.3):
    from anime_recommendations_amd import recs
    c = EC.planted()
    return c, recs.rp3_fit(c["user"], c["item"], np.ones(len(c["user"]), np.float32), c["n_users"], c["n_items"],
                           alpha=alpha, beta=beta, neighbours=neighbours)


@pytest.mark.parametrize("neighbours", [50, 0])
def test_rp3_fit_equals_the_restatement(neighbours):
    c, fit = _planted_fit(neighbours)
    want = R.rp3_fit(c["B"], 1.0, 0.3, neighbours)
    assert np.array_equal(_np(fit["pop"]), want["pop"]) and np.array_equal(_np(fit["deg"]), want["deg"])
    assert np.array_equal(_np(fit["user_q"]), want["user_q"]) and fit["scale"] == float(want["scale"])
    assert fit["n_liked"] == len(c["user"]) and fit["neighbours"] == neighbours
    if neighbours:
        assert np.array_equal(_np(fit["nbr_idx"]), want["nbr_idx"])
        assert np.array_equal(_u32(fit["nbr_sim"]), _u32(want["nbr_sim"]))
        top = float(np.nanmax(_np(fit["nbr_sim"])))
        assert "W" not in fit and not (_np(fit["nbr_idx"]) == np.arange(c["n_items"])[:, None]).any()
    else:
        assert np.array_equal(_u32(fit["W"]), _u32(want["W"])) and not _u32(fit["W"])[np.diag_indices(c["n_items"])].any()
        top = float(_np(fit["W"]).max())
    assert 256.0 <= top < 512.0


@pytest.mark.parametrize("neighbours", [50, 0])
def test_rp3_lists_ranks_and_neighbours_equal_the_restatement(neighbours):
    import torch
    from anime_recommendations_amd import ops, recs
    c, fit = _planted_fit(neighbours)
    n = c["n_items"]
    host = {k: _np(v) for k, v in fit.items() if hasattr(v, "detach")}
    off, hist = EC.planted_histories(c)
    n_l = len(off) - 1
    hw = (1.0 + (np.arange(len(hist)) % 9) / 8.0).astype(np.float32)                    # history weights up to 2
    seen_b = c["B"][:, c["held_user"]].T
    seen = _cuda(CR.pack_bits(seen_b).view(np.int32))
    for w in (None, hw):
        want_rows, err = R.rp3_scores(host, off, hist, w)
        assert err == 0
        rows = recs.rp3_rows_source(fit, off, hist, w)(0, n_l)
        assert np.array_equal(_u32(rows), _u32(want_rows))
        idx, sc = recs.rp3_topk(fit, off, hist, w, 10, seen, batch=97)
        wi, ws = CR.rows_topk(want_rows, 10, wbits=CR.pack_bits(seen_b))
        assert np.array_equal(_np(idx), wi) and np.array_equal(_u32(sc), _u32(ws))
        rank = _np(recs.rp3_rank(fit, off, hist, w, seen, np.arange(n_l), c["held_item"], batch=97))
        assert np.array_equal(rank, _np(ops.rows_rank(rows, np.arange(n_l), c["held_item"], seen)))
        if w is None:
            import ease_restatement as ER
            assert np.array_equal(rank, ER.ranks(want_rows, seen_b, np.arange(n_l), c["held_item"]))
            hr, pop_hr = EC.hit_rate(rank), EC.popularity_hit_rate(c)
            print("hit rate @10 (neighbours %d): RP3 %.4f, popularity %.4f" % (neighbours, hr, pop_hr))
            assert hr > pop_hr
    q = np.asarray([0, 5, n - 1, 5])
    keep = np.ones(n, np.uint8)
    keep[::7] = 0
    i1, s1 = recs.rp3_similar(fit, q, 8)
    wi, ws = R.rp3_similar(host, q, 8)
    assert np.array_equal(_np(i1), wi) and np.array_equal(_u32(s1), _u32(ws))
    assert not (_np(i1) == q[:, None]).any()
    i2, _ = recs.rp3_similar(fit, q, 8, keep=keep)
    assert (keep[_np(i2)[_np(i2) >= 0]] == 1).all() and not (_np(i2) == q[:, None]).any()
    with pytest.raises(ValueError, match="out of range"):
        recs.rp3_similar(fit, [n], 3)
    torch.cuda.synchronize()


# ---- the components, on the recs fixture ------------------------------------------------------------------------------
def _fixture_frames(rec):
    from anime_recommendations_amd import components as C
    return C.load_anime_df(RF.csv(rec, "anime_csv")), C.load_synopses(RF.csv(rec, "synopses_csv"))


def _argv(**kw):
    argv = []
    for k, v in kw.items():
        argv += ["--" + k, str(v)]
    return argv


def test_evaluate_baseline_rp3_on_the_recs_fixture(fixture_store, monkeypatch):  # noqa: F811
    import pandas as pd
    from anime_recommendations_amd import artifacts, components as C, data, recs, weights_io
    work, pq = fixture_store["work"], fixture_store["pq"]
    monkeypatch.chdir(work)
    ks = [1, 5, 20]
    par = {"alpha": 0.5, "beta": 0.6, "neighbours": 7, "min_rating": 0.5}
    ev = load_component("evaluate")
    argv = _argv(input_data="user_stats.parquet:latest", main_df_type="parquet", model="wandb_anime_nn.h5:latest",
                 model_type="h5", project_name="anime_recommendations", test_size=1000, eval_k=str(ks), min_rating=0.7,
                 eval_csv="rp3_metrics.csv", eval_type="eval_csv", ID_emb_name="user_embedding",
                 anime_emb_name="anime_embedding", baseline="popularity,rp3", **{"rp3_" + k: v for k, v in par.items()})
    _, summary = ev.go(ev.make_cli_parser().parse_args(argv))
    frame = pd.read_csv(work / "rp3_metrics.csv", float_precision="round_trip")
    assert frame.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity", "hit_rate_rp3",
                                      "ndcg_rp3"]
    assert {"rp3_mrr", "rp3_mean_rank", "rp3_hit_rate@5", "rp3_ndcg@20"} <= set(summary)
    logged = artifacts.artifact_metadata("rp3_metrics.csv:latest")
    assert logged["rp3_mrr"] == summary["rp3_mrr"]
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    table = data.load_user_stats(pq)
    pop_frame, pop = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline="popularity")
    assert frame[pop_frame.columns.tolist()].to_csv(index=False) == pop_frame.to_csv(index=False)
    assert {k: summary[k] for k in pop} == pop
    # the figures of the rp3_rank route on the training slice, and of the restatement's model of that slice
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    assert len(row) > 100
    tu, ta, tr = table.user[train], table.anime[train], table.rating[train]
    fit = recs.rp3_fit(tu, ta, tr, table.n_users, table.n_anime, 0.5, 0.5, 0.6, 7)
    hoff, hist, _ = recs.history_csr(tu, ta, tr, users, 0.5)
    seen = recs.listed_seen_bits(tu, ta, users, table.n_users, table.n_anime)
    rank = _np(recs.rp3_rank(fit, hoff, hist, None, seen, row, anime))
    b = recs.ranking_metrics(rank, ks)
    assert frame["hit_rate_rp3"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_rp3"].tolist() == [b["ndcg"][k] for k in ks]
    assert summary["rp3_mrr"] == b["mrr"] and summary["rp3_mean_rank"] == b["mean_rank"]
    liked = _np(tr).astype(np.float32) >= np.float32(0.5)
    B = np.zeros((table.n_anime, table.n_users), bool)
    B[_np(ta)[liked], _np(tu)[liked]] = True
    want = R.rp3_fit(B, 0.5, 0.6, 7)
    assert np.array_equal(_np(fit["nbr_idx"]), want["nbr_idx"]) and np.array_equal(_u32(fit["nbr_sim"]), _u32(want["nbr_sim"]))
    want_rows, err = R.rp3_scores(want, hoff, hist)
    seen_b = CR.unpack_bits(_np(seen).view(np.uint32), table.n_anime)
    import ease_restatement as ER
    assert err == 0 and np.array_equal(rank, ER.ranks(want_rows, seen_b, row, anime))


def test_hybrid_recs_component_takes_rp3_as_a_member(fixture_store, monkeypatch):  # noqa: F811
    import pandas as pd
    from anime_recommendations_amd import artifacts, components as C, weights_io
    work, rec, df = (fixture_store[k] for k in ("work", "rec", "df"))
    monkeypatch.chdir(work)
    flags = rec["flags"]
    user = int(rec["model_recs"]["cases"][0]["user"])
    mod = load_component("hybrid_recs")
    argv = _argv(project_name="anime_recommendations", model="wandb_anime_nn.h5:latest", model_type="h5",
                 main_df="user_stats.parquet:latest", main_df_type="parquet", anime_df="all_anime.csv:latest",
                 anime_df_type="raw_data", sypnopsis_df="synopses.csv:latest", sypnopsis_df_type="raw_data",
                 model_user_query=user, model_recs_fn="rp3.csv", model_num_recs=15, anime_types=flags["MR_TYPES"],
                 model_genres=flags["MR_GENRES"], model_recs_type="csv", flow_ID="user_id.csv:latest", flow_ID_type="csv",
                 random_user=False, save_model_recs=True, specify_types=True, specify_genres=False, model_ID_flow=False,
                 model_ID_conf=True, hybrid_systems="model,rp3")
    mod.go(mod.make_parser().parse_args(argv))
    got = pd.read_csv(work / ("User_ID_%d_hybrid_rp3.csv" % user))
    assert artifacts.artifact_metadata("hybrid_rp3.csv:latest")["hybrid_systems"] == ["model", "rp3"]
    assert len(got) == 15 and got.columns.tolist()[-3:] == ["Hybrid_score", "Rank_model", "Rank_rp3"]
    assert (got[["Rank_model", "Rank_rp3"]] >= 1).all().all() and (np.diff(got["Hybrid_score"]) <= 0).all()
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    anime_df, syn_df = _fixture_frames(rec)
    user_ids, anime_ids = C.index_tables(model, df)
    frame, stats = C.hybrid_recs_frame(model["U"], model["A"], weights_io.model_head(model), user_ids, anime_ids, df,
                                       anime_df, syn_df, user, 15, types=C.literal(flags["MR_TYPES"]),
                                       systems=("model", "rp3"))
    assert (work / ("User_ID_%d_hybrid_rp3.csv" % user)).read_text() == frame.to_csv(index=False)
    # the member's own ranks are those of the rp3 route under the list's mask
    small, _ = C.hybrid_recs_frame(model["U"], model["A"], weights_io.model_head(model), user_ids, anime_ids, df,
                                   anime_df, syn_df, user, 15, types=C.literal(flags["MR_TYPES"]), systems=("rp3",),
                                   rp3={"neighbours": 0, "beta": 0.0})
    assert small["Rank_rp3"].tolist() == list(range(1, 16))


def _rr_argv(flags, **kw):
    al = dict(project_name="anime_recommendations", main_df="user_stats.parquet:latest", main_df_type="parquet",
              anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopses_df="synopses.csv:latest",
              sypnopsis_df_type="raw_data", anime_query="none", a_query_number=20, random_anime=False,
              anime_rec_genres=flags["SA_GENRES"], an_spec_genres=False, types=flags["SA_TYPES"], spec_types=False,
              a_rec_type="csv", save_sim_anime=True)
    return _argv(**dict(al, **kw))


def test_rp3_recs_component_in_both_modes(fixture_store, monkeypatch):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, recs
    work, rec, df = (fixture_store[k] for k in ("work", "rec", "df"))
    anime_df, syn_df = _fixture_frames(rec)
    monkeypatch.chdir(work)
    mod = load_component("rp3_recs")
    parser = mod.make_parser()
    flags, query = rec["flags"], rec["similar_anime"]["cases"][0]["query"]
    types = C.literal(flags["SA_TYPES"])
    user_ids, anime_ids = C.index_tables({}, df)
    ui, ai, r = C.rating_indices(df, user_ids, anime_ids)
    meta = C.metadata_by_index(anime_ids, anime_df, syn_df)
    liked = _np(r).astype(np.float32) >= np.float32(0.5)
    B = np.zeros((len(anime_ids), len(user_ids)), bool)
    B[_np(ai)[liked], _np(ui)[liked]] = True
    # an anime query: the largest weights of the query's row, for the truncated and the dense model
    for neighbours in (30, 0):
        mod.go(parser.parse_args(_rr_argv(flags, anime_query=query, spec_types=True, rp3_neighbours=neighbours,
                                          rp3_beta=0.6, liked_min_rating=0.5)))
        fn = C.clean(query) + "_rp3.csv"
        got = (work / fn).read_text()
        logged = artifacts.artifact_metadata(fn + ":latest")
        frame, frame_fn, stats = C.rp3_similar_frame(df, anime_df, syn_df, query, 20, types=types, liked_min_rating=0.5,
                                                     beta=0.6, neighbours=neighbours)
        assert frame_fn == fn and got == frame.to_csv(index=False)
        assert logged["Queried anime"] == query and logged["beta"] == 0.6 and logged["neighbours"] == neighbours
        assert logged["liked_pairs"] == stats["liked_pairs"] == int(liked.sum()) and logged["alpha"] == 1.0
        assert frame.columns.tolist() == ["Name", "Similarity", "Genres", "Sypnopsis", "Episodes", "Japanese name",
                                          "Studios", "Premiered", "Score", "Type", "Source", "Rating"]
        assert 0 < len(frame) <= 20 and query not in frame["Name"].tolist() and frame["Type"].isin(types).all()
        assert (np.diff(frame["Similarity"]) <= 0).all()
        q = int(np.flatnonzero(np.asarray(anime_ids) == C.find_anime_id(query, anime_df))[0])
        want = R.rp3_fit(B, 1.0, 0.6, neighbours)
        keep = C.filter_mask(meta, anime_df, types)
        wi, wv = R.rp3_similar(want, [q], len(anime_ids) - 1)
        sel = [(j, v) for j, v in zip(wi[0], wv[0]) if j >= 0 and keep[j]][:20]
        assert frame["Name"].tolist() == meta["Name"].to_numpy()[[j for j, _ in sel]].tolist()
        assert np.array_equal(_u32(frame["Similarity"].to_numpy(np.float32)), _u32(np.asarray([v for _, v in sel], np.float32)))
    # a user query: that user's list among the anime they have not rated
    user = int(rec["model_recs"]["cases"][0]["user"])
    mod.go(parser.parse_args(_rr_argv(flags, user_query=user, rp3_neighbours=30)))
    got = (work / ("User_ID_%d_rp3_recs.csv" % user)).read_text()
    frame, stats = C.rp3_recs_frame(df, anime_df, syn_df, user, 20, neighbours=30)
    assert got == frame.to_csv(index=False) and len(frame) == 20 and "Rp3_score" in frame.columns
    assert artifacts.artifact_metadata("User_ID_%d_rp3_recs.csv:latest" % user)["neighbours"] == 30
    mine = df[df.user_id == user]
    assert not set(frame["anime_id"]) & set(mine.anime_id) and (np.diff(frame["Rp3_score"]) <= 0).all()
    B0 = np.zeros((len(anime_ids), len(user_ids)), bool)
    B0[_np(ai), _np(ui)] = True
    want = R.rp3_fit(B0, 1.0, 0.3, 30)
    pos = {a: i for i, a in enumerate(np.asarray(anime_ids).tolist())}
    urow = int(np.flatnonzero(np.asarray(user_ids) == user)[0])
    hoff, hist, _ = recs.history_csr(ui, ai, r, [urow])
    assert sorted(hist.tolist()) == sorted(pos[a] for a in mine.anime_id)
    scores, err = R.rp3_scores(want, hoff, hist)
    seen = np.zeros((1, len(anime_ids)), bool)
    seen[0, [pos[a] for a in mine.anime_id]] = True
    wi, wv = CR.rows_topk(scores, 20, keep=meta["has_meta"].to_numpy().astype(np.uint8), wbits=CR.pack_bits(seen))
    assert err == 0 and frame["anime_id"].tolist() == np.asarray(anime_ids)[wi[0]].tolist()
    assert np.array_equal(_u32(frame["Rp3_score"].to_numpy(np.float32)), _u32(wv[0]))
    with pytest.raises(ValueError, match="exactly one"):
        mod.go(parser.parse_args(_rr_argv(flags, user_query=user, anime_query="Naruto")))
