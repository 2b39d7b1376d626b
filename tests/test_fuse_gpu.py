"""GPU tests of the hybrid lists (anirec_fuse_rows; ops.fuse_rows, recs.hybrid_topk / hybrid_rank,
components.hybrid_recs_frame, the hybrid_recs component and evaluate --baseline hybrid).

Yardstick: the NumPy restatement (tests/fuse_restatement.py).  Every comparison is equality of the uint32 views of the
fp32 results, NaNs included; there is no tolerance anywhere.

Shapes: the smallest at which a kernel can go wrong — row lengths around the wave (64), around the largest workgroup
(1024: from there a thread holds more than one item), past the next power of two (2049: virtual padding of the sort
network), and the two bounds of the network and of the LDS image (20 479, 20 480) with two rows only."""
import ctypes
import json

import numpy as np
import pandas as pd
import pytest

import cooc_restatement as CR
import fuse_restatement as R
import poison
import recs_fixture as RF
from test_cooc_gpu import fixture_store  # noqa: F401  (the recs fixture as an artifact store)
from test_fuse_cpu import expected_hybrid_frame
from test_rank_gpu import _run as _run_out
from test_recs_fixtures_gpu import _run

pytestmark = pytest.mark.gpu
N_ITEMS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049)
KINDS = ("normal", "four", "equal", "zeros", "special", "nan", "wide")
METHODS = ("rrf", "minmax")


def _cuda(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    g, w = _bits(got.cpu().numpy() if hasattr(got, "cpu") else got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert not len(bad), (what, len(bad), bad[:5].tolist(), g[g != w][:5].tolist(), w[g != w][:5].tolist())


def _content(kind, shape, rng):
    """row contents that can break the order or the arithmetic"""
    if kind == "normal":
        return rng.standard_normal(shape).astype(np.float32)
    if kind == "four":                                          # mass ties
        return rng.choice(np.float32([0.25, 0.5, -1.0, 2.0]), shape)
    if kind == "equal":
        return np.full(shape, np.float32(0.75))
    if kind == "zeros":                                         # +0 above -0
        return rng.choice(np.float32([0.0, -0.0]), shape)
    if kind == "nan":                                           # a system that says nothing
        return np.full(shape, np.nan, np.float32)
    x = rng.standard_normal(shape).astype(np.float32)
    if kind == "special":
        hit = rng.random(shape) < 0.2
        x[hit] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0]), int(hit.sum()))
        return x
    x[rng.random(shape) < 0.3] = np.float32(3e38)                # "wide": hi - lo overflows
    x[rng.random(shape) < 0.3] = np.float32(-3e38)
    return x


def _systems(nq, n, kinds, rng, shared=(), pad=()):
    """(device rows, host rows): system s of kind kinds[s]; s in ``shared`` a 1-D vector, s in ``pad`` with ld = n + 5
    and poison in the padding (the restatement reads the first n columns alone)"""
    dev, host = [], []
    for s, kind in enumerate(kinds):
        if s in shared:
            x = _content(kind, (n,), rng)
        elif s in pad:
            x = np.concatenate([_content(kind, (nq, n), rng), np.full((nq, 5), np.float32(np.inf))], axis=1)
        else:
            x = _content(kind, (nq, n), rng)
        dev.append(_cuda(x))
        host.append(x)
    return dev, host


def _masks(nq, n, rng):
    """watched bits with garbage past n, a row with every bit set and a row with none; a keep mask"""
    W = rng.random((nq, n)) < 0.3
    W[0] = True
    if nq > 1:
        W[1] = False
    bits = CR.pack_bits(W).copy()
    if n % 32:
        bits[:, -1] |= (rng.integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)
                        & np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF))
    keep = (rng.random(n) < 0.8).astype(np.uint8)
    return W, bits, keep


def _fuse(dev, weights, method, c, n, bits=None, keep=None):
    from anime_recommendations_amd import ops
    return ops.fuse_rows(dev, weights, method, c, n=n, wbits=None if bits is None else _cuda(bits.view(np.int32)),
                         keep=None if keep is None else _cuda(keep))


# ---- the kernel against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", N_ITEMS)
def test_fuse_rows_equals_the_restatement(n, method):
    rng = np.random.default_rng(1000 * n + len(method))
    m = R.METHODS[method]
    # one system, one row, no masks, c = 0
    for kind in KINDS:
        dev, host = _systems(1, n, [kind], rng)
        _same(_fuse(dev, None, method, 0, n), R.fuse_rows(host, None, m, 0, n), ("solo", kind))
    # two systems, three rows: masks, a shared vector, ld > n with poison in the padding, unequal weights
    for kinds in (("normal", "four"), ("special", "zeros"), ("wide", "equal"), ("nan", "normal")):
        dev, host = _systems(3, n, kinds, rng, shared=(1,), pad=(0,))
        W, bits, keep = _masks(3, n, rng)
        got = _fuse(dev, [0.5, 3.0], method, 60, n, bits, keep)
        _same(got, R.fuse_rows(host, [0.5, 3.0], m, 60, n, bits, keep), ("pair", kinds))
        E = ~W & (keep != 0)[None]
        assert np.array_equal(_bits(got.cpu().numpy())[~E], np.full(int((~E).sum()), 0x7FC00000, np.uint32))
    # three systems over 67 rows, a weight of 0; eight systems over three rows
    dev, host = _systems(67, n, ("normal", "special", "four"), rng, pad=(2,))
    W, bits, keep = _masks(67, n, rng)
    for w in ([1.0, 0.0, 2.5], None):
        _same(_fuse(dev, w, method, 60, n, bits), R.fuse_rows(host, w, m, 60, n, bits), ("three", w))
    dev, host = _systems(3, n, KINDS + ("normal",), rng, shared=(3,))
    w8 = [1, 0, 0.25, 3, 1e-30, 3e38, 2, 1]
    _same(_fuse(dev, w8, method, 0, n, None, keep), R.fuse_rows(host, w8, m, 0, n, None, keep), "eight")


@pytest.mark.parametrize("n", (20479, 20480))
def test_the_longest_rows(n):
    """the bounds of the sort network and of the LDS image: two rows only"""
    rng = np.random.default_rng(n)
    dev, host = _systems(2, n, ("special", "four"), rng, shared=(1,))
    W, bits, keep = _masks(2, n, rng)
    W[0] = rng.random(n) < 0.1
    bits = CR.pack_bits(W)
    for method in METHODS:
        got = _fuse(dev, [1.0, 0.5], method, 60, n, bits, keep)
        _same(got, R.fuse_rows(host, [1.0, 0.5], R.METHODS[method], 60, n, bits, keep), method)


def test_a_longer_row_is_refused_without_a_launch():
    import torch
    from anime_recommendations_amd import ops
    x = torch.zeros(1, 20481, dtype=torch.float32, device="cuda:0")
    with pytest.raises(ValueError, match="1 .. 20480"):
        ops.fuse_rows([x])
    with pytest.raises(ValueError, match="1 .. 8"):
        ops.fuse_rows([x[:, :10]] * 9)
    with pytest.raises(ValueError, match="shortest row"):
        ops.fuse_rows([x[:, :10].contiguous()], n=11)
    with pytest.raises(ValueError, match="same number of rows"):
        ops.fuse_rows([x[:, :10].contiguous(), torch.zeros(2, 10, device="cuda:0")])
    assert tuple(ops.fuse_rows([torch.zeros(0, 10, device="cuda:0")]).shape) == (0, 10)


@pytest.mark.parametrize("method", METHODS)
def test_output_pitch_padding_and_dirty_buffers(method):
    """columns n .. ld_out are not written, and what the output held changes nothing: the same call twice"""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    nq, n, ld_out = 5, 1025, 1031
    dev, host = _systems(nq, n, ("normal", "special", "four"), rng, shared=(2,))
    W, bits, keep = _masks(nq, n, rng)
    wb, kp = _cuda(bits.view(np.int32)), _cuda(keep)
    want = R.fuse_rows(host, [1, 2, 0.5], R.METHODS[method], 7, n, bits, keep)
    out = torch.empty(nq, ld_out, dtype=torch.float32, device="cuda:0")
    ptrs = (ctypes.c_void_p * 3)(*[r.data_ptr() for r in dev])
    lds = (ctypes.c_int64 * 3)(n, n, 0)
    wts = (ctypes.c_float * 3)(1, 2, 0.5)
    for byte in poison.ORDER:
        poison.fill(out, byte)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.anirec_fuse_rows(ptrs, lds, 3, n, nq, _lib.ptr(wb), _lib.ptr(kp), wts, R.METHODS[method], 7,
                                    _lib.ptr(out), ld_out, s) == 0
        got = out.cpu().numpy()
        _same(got[:, :n], want, (method, byte))
        assert (got[:, n:].view(np.uint8) == byte).all(), (method, byte)


def test_fuse_rows_replays_from_a_graph():
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(8)
    nq, n = 4, 1025
    dev, host = _systems(nq, n, ("normal", "four"), rng)
    W, bits, _ = _masks(nq, n, rng)
    wb = _cuda(bits.view(np.int32))
    out = {m: torch.empty(nq, n, dtype=torch.float32, device="cuda:0") for m in METHODS}
    for o in out.values():
        poison.fill(o, 0x3F)
    ptrs = (ctypes.c_void_p * 2)(*[r.data_ptr() for r in dev])
    lds, wts = (ctypes.c_int64 * 2)(n, n), (ctypes.c_float * 2)(1, 2)
    _fuse(dev, [1, 2], "rrf", 60, n, bits)                      # the eager call first: attributes set outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st = [lib.anirec_fuse_rows(ptrs, lds, 2, n, nq, _lib.ptr(wb), None, wts, R.METHODS[m], 60, _lib.ptr(out[m]), n, s)
              for m in METHODS]
    assert st == [0, 0]
    torch.cuda.synchronize()
    assert all(bool((o.view(torch.uint8) == 0x3F).all()) for o in out.values())      # captured, not run
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for m in METHODS:
            _same(out[m], R.fuse_rows(host, [1, 2], R.METHODS[m], 60, n, bits), ("replay", m))
            poison.fill(out[m], 0x7F)


# ---- properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (65, 1025, 2049))
def test_one_system_under_rrf_keeps_that_systems_order(n):
    """tests/test_fuse_cpu.py shows that an RRF term falls strictly with the rank; so the fused row of one system lists the
    items as the system's own row does, ties and NaNs included"""
    import torch
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(n)
    W, bits, keep = _masks(3, n, rng)
    wb, kp = _cuda(bits.view(np.int32)), _cuda(keep)
    for kind in ("normal", "four", "special", "zeros"):
        x = _cuda(_content(kind, (3, n), rng))
        for c, w in ((0, 1.0), (60, 1e-30), (1 << 20, 3e38)):
            fused = ops.fuse_rows([x], [w], "rrf", c, wbits=wb, keep=kp)
            got = ops.rows_topk(fused, n, keep=kp, wbits=wb)[0]
            assert torch.equal(got, ops.rows_topk(x, n, keep=kp, wbits=wb)[0]), (kind, c, w)


@pytest.fixture(scope="module")
def recs_table(tmp_path_factory):
    from anime_recommendations_amd import components as C, data, weights_io
    work = tmp_path_factory.mktemp("fuse")
    rec = RF.load()
    z, df = rec["npz"], RF.ratings(rec)
    user_ids, anime_ids = C.index_tables({}, df)
    pq, mp = str(work / "user_stats.parquet"), str(work / "wandb_anime_nn.h5")
    df.to_parquet(pq, index=False)
    weights_io.save_model(mp, z["U"], z["A"], dict(rec["model_recs"]["heads"]["sigmoid"], activation="sigmoid"),
                          user_ids=user_ids, anime_ids=anime_ids)
    return weights_io.load_model(mp), data.load_user_stats(pq)


ALS_PAR = dict(factors=32, sweeps=2, cg_steps=2, alpha=4.0, reg=0.05, min_rating=0.6, seed=3)
KNN_PAR = dict(neighbours=20, measure="jaccard", shrink=10.5, min_support=2, min_rating=0.6)


def _members(model, table, users, train):
    """(sources by name, seen bits) of the four systems on the training slice, fitted as evaluate_frame fits them"""
    import torch
    from anime_recommendations_amd import recs, weights_io
    tu, ta, tr = (np.asarray(c[train]) for c in (table.user, table.anime, table.rating))
    seen = recs.listed_seen_bits(tu, ta, users, table.n_users, table.n_anime)
    tU, tA = torch.as_tensor(np.asarray(model["U"])).cuda(), torch.as_tensor(np.asarray(model["A"])).cuda()
    knn = recs.itemknn_fit(tu, ta, tr, table.n_users, table.n_anime, KNN_PAR["min_rating"], KNN_PAR["neighbours"],
                           KNN_PAR["measure"], KNN_PAR["shrink"], KNN_PAR["min_support"])
    off, hist, _ = recs.history_csr(tu, ta, tr, users, min_rating=KNN_PAR["min_rating"])
    liked = tr.astype(np.float32) >= np.float32(ALS_PAR["min_rating"])
    fit = recs.als_fit(tu[liked], ta[liked], table.n_users, table.n_anime, 32, 2, 2, 4.0, 0.05, seed=3)
    return {"model": (recs.model_rows_source(tU, tA, weights_io.model_head(model), users), (tU, tA)),
            "popularity": (recs.popularity_scores(ta, table.n_anime, table.n_users).cuda(), None),
            "itemknn": (recs.itemknn_rows_source(knn, off, hist), (knn, off, hist)),
            "als": (recs.als_rows_source(fit, users), fit)}, seen


def test_hybrid_rank_of_one_member_is_that_members_own_rank(recs_table):
    import torch
    from anime_recommendations_amd import ops, recs, weights_io
    model, table = recs_table
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    assert len(row) > 100
    members, seen = _members(model, table, users, train)
    (tU, tA), (knn, off, hist), fit = members["model"][1], members["itemknn"][1], members["als"][1]
    own = {"model": ops.predict_rank(tU, tA, weights_io.model_head(model), users, row, anime, watched_bits=seen)[0],
           "popularity": ops.score_rank(members["popularity"][0], len(users), row, anime, watched_bits=seen),
           "itemknn": recs.itemknn_rank(knn, off, hist, None, seen, row, anime),
           "als": recs.als_rank(fit, users, seen, row, anime)}
    for name, want in own.items():
        for c, batch in ((60, recs.HYBRID_BATCH), (0, 5)):
            got = recs.hybrid_rank([members[name][0]], seen, row, anime, rrf_c=c, batch=batch)
            assert got.dtype == torch.int32 and torch.equal(got, want), (name, c, batch)
    # all four, both methods: the restatement's fusion of the members' own rows, ranked by the restatement
    rows = [src(0, len(users)).cpu().numpy() if callable(src) else src.cpu().numpy() for src, _ in members.values()]
    sb = seen.cpu().numpy().view(np.uint32)
    for method in METHODS:
        w = [1.0, 0.25, 2.0, 1.0]
        got = recs.hybrid_rank([src for src, _ in members.values()], seen, row, anime, w, method, 60, batch=6)
        fused = R.fuse_rows(rows, w, R.METHODS[method], 60, table.n_anime, sb)
        assert np.array_equal(got.cpu().numpy(), CR.ops_rows_rank(fused, row, anime, sb)), method
        idx, sc = recs.hybrid_topk([src for src, _ in members.values()], 12, w, method, 60, seen, batch=4)
        want_i, want_s = CR.rows_topk(fused, 12, wbits=sb)
        assert np.array_equal(idx.cpu().numpy(), want_i)
        _same(sc, want_s, ("topk", method))
    t0 = int(np.flatnonzero((sb[row, anime >> 5] >> (anime & 31).astype(np.uint32)) & 1 == 0)[0])
    wrong = seen.clone()
    wrong[int(row[t0]), int(anime[t0]) >> 5] |= int(np.int32(np.uint32(1 << (int(anime[t0]) & 31)).view(np.int32)))
    with pytest.raises(ValueError, match="own watched bit"):
        recs.hybrid_rank([members["model"][0]], wrong, row, anime)


# ---- the components, end to end on the recs fixture -------------------------------------------------------------------
def _mr_flags(flags, user, n_recs, fn):
    return dict(project_name="anime_recommendations", model="wandb_anime_nn.h5:latest", model_type="h5",
                main_df="user_stats.parquet:latest", main_df_type="parquet", anime_df="all_anime.csv:latest",
                anime_df_type="raw_data", sypnopsis_df="synopses.csv:latest", sypnopsis_df_type="raw_data",
                model_user_query=user, model_recs_fn=fn, model_num_recs=n_recs, anime_types=flags["MR_TYPES"],
                model_genres=flags["MR_GENRES"], model_recs_type="csv", flow_ID="user_id.csv:latest", flow_ID_type="csv",
                random_user=False, save_model_recs=True, specify_types=True, specify_genres=False, model_ID_flow=False,
                model_ID_conf=True)


def test_hybrid_recs_component_on_the_recs_fixture(fixture_store):  # noqa: F811
    import torch
    from anime_recommendations_amd import artifacts, components as C, ops, recs, weights_io
    work, env, rec, df = (fixture_store[k] for k in ("work", "env", "rec", "df"))
    flags = rec["flags"]
    user = int(rec["model_recs"]["cases"][0]["user"])
    _run("hybrid_recs", dict(_mr_flags(flags, user, 15, "recs.csv"), hybrid_weights="[1, 0.5, 2]", hybrid_rrf_c=10), str(work),
         env)
    fn = "User_ID_%d_hybrid_recs.csv" % user
    got = (work / fn).read_text()
    meta = artifacts.artifact_metadata("hybrid_recs.csv:latest")
    stats = {"hybrid_systems": ["model", "itemknn", "als"], "hybrid_weights": [1.0, 0.5, 2.0], "hybrid_method": "rrf",
             "hybrid_rrf_c": 10}
    assert {k: meta[k] for k in stats} == stats and meta["Filename"] == fn and meta["Queried user: "] == user
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    anime_df = C.load_anime_df(RF.csv(rec, "anime_csv"))
    syn_df = C.load_synopses(RF.csv(rec, "synopses_csv"))
    user_ids, anime_ids = C.index_tables(model, df)
    tables = (model["U"], model["A"], weights_io.model_head(model), user_ids, anime_ids, df, anime_df, syn_df)
    kw = dict(types=C.literal(flags["MR_TYPES"]), weights=[1, 0.5, 2], rrf_c=10)
    frame, got_stats = C.hybrid_recs_frame(*tables, user, 15, **kw)
    assert got == frame.to_csv(index=False) and got_stats == stats
    # the frame from the restatements: fusion, select and ranks in NumPy, the item-kNN member too; the model's grid and
    # the ALS fit (not what is under test here) are the GPU's
    tU, tA = torch.as_tensor(model["U"]).cuda(), torch.as_tensor(model["A"]).cuda()

    def grid(us):
        return ops.predict_grid(tU, tA, tables[2], us).cpu().numpy()

    def als_rows(ui, ai, par, row):
        fit = recs.als_fit(ui, ai, len(user_ids), len(anime_ids), par["factors"], int(par["sweeps"]), par["cg_steps"],
                           par["alpha"], par["reg"], seed=int(par["seed"]))
        return ops.dot_scores(fit["X"][[row]], fit["Y"]).cpu().numpy()
    want, want_stats = expected_hybrid_frame(*tables, user, 15, grid, als_rows, **kw)
    assert got == want.to_csv(index=False) and want_stats == stats
    assert len(want) == 15 and want["Type"].isin(C.literal(flags["MR_TYPES"])).all()
    assert (np.diff(want["Hybrid_score"]) <= 0).all() and (want[["Rank_model", "Rank_itemknn", "Rank_als"]] >= 1).all().all()
    # one member: model_recs' anime in model_recs' order
    _run("hybrid_recs", dict(_mr_flags(flags, user, 40, "solo.csv"), hybrid_systems="model"), str(work), env)
    _run("model_recs", _mr_flags(flags, user, 40, "plain.csv"), str(work), env)
    solo = pd.read_csv(work / ("User_ID_%d_hybrid_solo.csv" % user))
    plain = pd.read_csv(work / ("User_ID_%d_plain.csv" % user))
    assert len(plain) == 40 and solo["anime_id"].tolist() == plain["anime_id"].tolist()
    assert solo["Rank_model"].tolist() == list(range(1, 41))
    assert solo.columns.tolist() == plain.columns.tolist() + ["Hybrid_score", "Rank_model"]


def test_evaluate_baseline_hybrid_on_the_recs_fixture(fixture_store):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, data, recs, weights_io
    work, env, pq = fixture_store["work"], fixture_store["env"], fixture_store["pq"]
    ks = [1, 5, 20]
    ev = dict(input_data="user_stats.parquet:latest", main_df_type="parquet", model="wandb_anime_nn.h5:latest",
              model_type="h5", project_name="anime_recommendations", test_size=1000, eval_k=str(ks), min_rating=0.7,
              eval_csv="hybrid_metrics.csv", eval_type="eval_csv", ID_emb_name="user_embedding",
              anime_emb_name="anime_embedding", baseline="popularity,hybrid", ci_replicates=200,
              hybrid_systems="model,popularity,itemknn,als", hybrid_weights="[1, 0.25, 2, 1]")
    ev.update({"itemknn_" + k: v for k, v in KNN_PAR.items()})
    ev.update({"als_" + k: v for k, v in ALS_PAR.items()})
    code, out = _run_out("evaluate", ev, str(work), env)
    assert code == 0, out[-3000:]
    summary = json.loads(out.strip().splitlines()[-1])
    frame = pd.read_csv(work / "hybrid_metrics.csv", float_precision="round_trip")
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    table = data.load_user_stats(pq)
    # without the hybrid the frame and the summary are what they were
    pop_frame, pop = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline="popularity", ci_replicates=200)
    assert frame[pop_frame.columns.tolist()].to_csv(index=False) == pop_frame.to_csv(index=False)
    assert {k: summary[k] for k in pop} == pop
    assert frame.columns.tolist()[:7] == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity",
                                          "hit_rate_hybrid", "ndcg_hybrid"]
    # the hybrid columns, intervals and paired p-values from hybrid_rank's ranks through recs.bootstrap_metrics
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    members, seen = _members(model, table, users, train)
    import torch
    from anime_recommendations_amd import ops
    tU, tA = members["model"][1]
    rank = ops.predict_rank(tU, tA, weights_io.model_head(model), users, row, anime, watched_bits=seen)[0]
    pop_rank = ops.score_rank(members["popularity"][0], len(users), row, anime, watched_bits=seen)
    hyb = recs.hybrid_rank([src for src, _ in members.values()], seen, row, anime, [1, 0.25, 2, 1], "rrf", 60)
    b = recs.ranking_metrics(hyb, ks)
    assert frame["hit_rate_hybrid"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_hybrid"].tolist() == [b["ndcg"][k] for k in ks]
    assert summary["hybrid_mrr"] == b["mrr"] and summary["hybrid_mean_rank"] == b["mean_rank"]
    boot = recs.bootstrap_metrics({"model": rank, "popularity": pop_rank, "hybrid": hyb}, row, len(users), ks, 200, 0, 0.95,
                                  unit_key=users, n_rows=table.n_anime)
    for i, k in enumerate(ks):
        for metric in ("hit_rate", "ndcg"):
            fig, d = boot["figures"]["hybrid"]["%s@%d" % (metric, k)], boot["diffs"]["hybrid"]["%s@%d" % (metric, k)]
            assert frame["%s_hybrid_lo" % metric][i] == fig["lo"] and frame["%s_hybrid_hi" % metric][i] == fig["hi"]
            assert frame["%s_diff_hybrid" % metric][i] == d["diff"] and frame["%s_p_hybrid" % metric][i] == d["p"]
            assert frame["%s_diff_hybrid_lo" % metric][i] == d["lo"] and frame["%s_diff_hybrid_hi" % metric][i] == d["hi"]
    for key in ("mrr", "mean_rank"):
        assert summary["hybrid_%s_lo" % key] == boot["figures"]["hybrid"][key]["lo"]
        assert summary["%s_diff_hybrid" % key] == boot["diffs"]["hybrid"][key]["diff"]
        assert summary["%s_p_hybrid" % key] == boot["diffs"]["hybrid"][key]["p"]
    assert summary["ci_replicates"] == 200 and 0 < summary["mrr_p_hybrid"] <= 1
