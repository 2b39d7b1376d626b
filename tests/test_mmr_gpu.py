"""GPU tests of the greedy MMR re-rank (anirec_mmr_rerank, ops.mmr_rerank, recs.diverse_topk, the diverse_recs component).

Yardstick: the NumPy restatement (tests/mmr_restatement.py) run on the similarities the existing ``ops.cosine_scores``
returns for the same normalised table — that kernel is not under test here, and the header defines sim(i, j) as its
chain, bit for bit.  Every comparison of idx, pos, the score bits and the pen bits is exact.

Shapes: widths 32, 64, 128, 256; n_cand 1, 2, 63, 64, 65 (a wave and one past it), 100, and anirec_mmr_max_cand(width)
(1024 .. 128: two to four candidates per lane at widths 32 and 64, the full LDS image); k 1, 10 and n_cand; lam 0, 0.3
and 1; a 777-row table; 37 lists a call, the first of them with the special content ``_lists`` plants.  The re-rank is
greedy, so the reference for k = n_cand is computed once per (width, n_cand, lam) and its first columns are the
reference for the smaller k.
"""
import ctypes
import json
import os

import numpy as np
import pandas as pd
import pytest

import mmr_restatement as M
import poison
from test_components_gpu import _run, pipeline  # noqa: F401  (the components' pipeline fixture, as it is)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, N_LISTS = 777, 37
TWIN_A, TWIN_B, ZERO_ROW = 5, 9, 11        # two bit-identical table rows and a zero row (NaN once normalised)
WIDTHS = (32, 64, 128, 256)
N_CANDS = (1, 2, 63, 64, 65, 100, "max")
LAMS = (0.0, 0.3, 1.0)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_TABLES = {}


def _table(dim):
    """(What on the device, What on the host, Sfull [N_ROWS, N_ROWS]: row q = ops.cosine_scores(What, q)), once a width"""
    if dim not in _TABLES:
        from anime_recommendations_amd import ops
        rng = np.random.default_rng(100 + dim)
        W = rng.normal(size=(N_ROWS, dim)).astype(np.float32)
        W[TWIN_B] = W[TWIN_A]
        W[ZERO_ROW] = 0
        Wh = ops.rownorm(_cuda(W))
        Wh_host = Wh.cpu().numpy()
        assert np.isnan(Wh_host[ZERO_ROW]).all() and np.array_equal(_bits(Wh_host[TWIN_A]), _bits(Wh_host[TWIN_B]))
        S = np.stack([ops.cosine_scores(Wh, q).cpu().numpy() for q in range(N_ROWS)])
        _TABLES[dim] = (Wh, Wh_host, S)
    return _TABLES[dim]


def _lists(dim, n_cand, seed=0):
    """N_LISTS candidate lists: random rows and N(0, 1) scores (both signs: at lam = 0 the products are -0 and +0), the
    first ones with the content that takes a path of its own, as far as n_cand has room for it."""
    rng = np.random.default_rng(seed * 1000 + dim + n_cand)
    idx = rng.integers(0, N_ROWS, (N_LISTS, n_cand)).astype(np.int32)
    idx[idx == ZERO_ROW] = ZERO_ROW + 1
    score = rng.normal(size=(N_LISTS, n_cand)).astype(np.float32)
    mid = n_cand // 2
    idx[0, [0, mid, n_cand - 1]] = -1                           # empty slots at the front, the middle and the end
    score[1, [0, mid]] = np.nan                                 # NaN scores
    idx[3, 0] = ZERO_ROW                                        # a zero table row
    idx[4, : n_cand - 1] = -1                                   # fewer than k present candidates (one, or none)
    idx[5, :] = -1                                              # nothing present at all
    score[6, :] = 0.5                                           # every score tied
    if n_cand >= 2:
        idx[2, 1], score[2, 1] = idx[2, 0], score[2, 0]         # a repeated index, tied with itself
        idx[7, 0], idx[7, n_cand - 1] = TWIN_B, TWIN_A          # two bit-identical rows with one score
        score[7, 0] = score[7, n_cand - 1] = 10.0
        score[8, 0], score[8, 1] = np.inf, -np.inf
    return idx, score


def _n_cand(dim, n_cand):
    from anime_recommendations_amd import _lib
    return _lib.mmr_max_cand(dim) if n_cand == "max" else n_cand


_REFS = {}


def _reference(dim, n_cand, lam, seed=0):
    """the restatement for k = n_cand (its first k columns are the reference for any smaller k), once per shape"""
    key = (dim, n_cand, lam, seed)
    if key not in _REFS:
        _, Wh_host, S = _table(dim)
        idx, score = _lists(dim, n_cand, seed)
        _REFS[key] = M.rerank_lists(S, Wh_host, idx, score, n_cand, lam)
    return _REFS[key]


def _same(got, ref, k, what):
    gi, gp, gs, gn = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in got]
    assert np.array_equal(gi, ref[0][:, :k]), what
    assert np.array_equal(gp, ref[1][:, :k]), what
    assert np.array_equal(_bits(gs), _bits(ref[2][:, :k])), what
    assert np.array_equal(_bits(gn), _bits(ref[3][:, :k])), what


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("n_cand", N_CANDS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_rerank_equals_the_restatement(dim, n_cand, lam):
    from anime_recommendations_amd import ops
    n_cand = _n_cand(dim, n_cand)
    Wh, _, _ = _table(dim)
    idx, score = _lists(dim, n_cand)
    ref = _reference(dim, n_cand, lam)
    for k in sorted({1, min(10, n_cand), n_cand}):
        got = ops.mmr_rerank(Wh, _cuda(idx), _cuda(score), k, lam)
        _same(got, ref, k, (dim, n_cand, k, lam))
    # the planted content did what it is there for (checked on the reference, which the kernel has just equalled)
    ri, rp, rs, rn = ref
    assert (ri[5] == -1).all() and np.isnan(rs[5]).all() and np.isnan(rn[5]).all()
    assert rp[4, 0] == n_cand - 1 and (rp[4, 1:] == -1).all()                # one present candidate, then the padding
    assert ZERO_ROW not in ri[3].tolist() and (rp[0] >= 0).sum() == max(0, n_cand - len({0, n_cand // 2, n_cand - 1}))
    if n_cand >= 2:
        assert rp[7, 0] == 0                                    # the twins tie at the top score: the lower position first
        if lam == 1.0:
            assert rp[7, :2].tolist() == [0, n_cand - 1] and rp[6].tolist() == list(range(n_cand))
            assert rp[2].tolist().index(1) == rp[2].tolist().index(0) + 1     # the repeated index: two adjacent picks
            assert rp[8, 0] == 0 and rp[8, -1] == 1                           # +inf first, -inf last


def test_a_list_does_not_depend_on_its_context():
    """a list run alone, at another position among other lists, and twice: the same bits"""
    from anime_recommendations_amd import ops
    dim, n_cand, k, lam = 128, 100, 10, 0.3
    Wh, _, _ = _table(dim)
    idx, score = _lists(dim, n_cand)
    ref = _reference(dim, n_cand, lam)
    ci, cs = _cuda(idx), _cuda(score)
    first = ops.mmr_rerank(Wh, ci, cs, k, lam)
    _same(first, ref, k, "whole call")
    _same(ops.mmr_rerank(Wh, ci, cs, k, lam), ref, k, "second run")
    perm = np.random.default_rng(5).permutation(N_LISTS)
    moved = ops.mmr_rerank(Wh, _cuda(idx[perm]), _cuda(score[perm]), k, lam)
    _same(moved, [r[perm] for r in ref], k, "permuted call")
    for l in (0, 7, 20, 36):
        alone = ops.mmr_rerank(Wh, ci[l:l + 1].clone(), cs[l:l + 1].clone(), k, lam)
        _same(alone, [r[l:l + 1] for r in ref], k, "list %d alone" % l)


@pytest.mark.parametrize("byte", poison.ORDER)
def test_dirty_outputs_are_fully_overwritten(byte):
    from anime_recommendations_amd import ops
    for dim, n_cand, k, lam in ((32, 65, 65, 0.3), (128, 100, 10, 0.3)):
        Wh, _, _ = _table(dim)
        idx, score = _lists(dim, n_cand)
        ci, cs = _cuda(idx), _cuda(score)
        log = []
        with poison.poisoned(byte, log):
            got = ops.mmr_rerank(Wh, ci, cs, k, lam)
        assert len(log) == 5 and sum(log) == 4 * N_LISTS * k * 4 + 4       # the four outputs and the flag word
        _same(got, _reference(dim, n_cand, lam), k, (byte, dim))


def _raw(dim, idx, score, k, lam, n_rows=N_ROWS, n_lists=None, n_cand=None, null=None, fill=0x3F, dim_arg=None):
    """anirec_mmr_rerank itself, its outputs and flag pre-filled with ``fill`` bytes: no wrapper check between the
    test and the entry point.  ``null``: the name of one pointer passed as NULL.  Returns (status, outs, err)."""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    Wh = _table(dim)[0]
    ci, cs = _cuda(idx), _cuda(score)
    shape = (idx.shape[0], max(k, 1))
    outs = [poison.fill(torch.empty(shape, dtype=dt, device="cuda"), fill)
            for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), fill)
    p = dict(What=Wh, cand_idx=ci, cand_score=cs, out_idx=outs[0], out_pos=outs[1], out_score=outs[2], out_pen=outs[3],
             err=err)
    if null:
        p[null] = None
    st = lib.anirec_mmr_rerank(_lib.ptr(p["What"]), dim if dim_arg is None else dim_arg, n_rows, _lib.ptr(p["cand_idx"]),
                               _lib.ptr(p["cand_score"]), idx.shape[0] if n_lists is None else n_lists,
                               idx.shape[1] if n_cand is None else n_cand, k, lam, _lib.ptr(p["out_idx"]),
                               _lib.ptr(p["out_pos"]), _lib.ptr(p["out_score"]), _lib.ptr(p["out_pen"]),
                               _lib.ptr(p["err"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, outs, err


@pytest.mark.parametrize("bad_value", [N_ROWS, -2, 2 ** 31 - 1])
def test_a_bad_index_poisons_its_own_list_alone(bad_value):
    dim, n_cand, k, lam = 64, 65, 10, 0.3
    idx, score = _lists(dim, n_cand)
    ref = [r.copy() for r in _reference(dim, n_cand, lam)]
    idx = idx.copy()
    idx[20, 64] = bad_value
    ref[0][20], ref[1][20], ref[2][20], ref[3][20] = -1, -1, np.nan, np.nan
    st, outs, err = _raw(dim, idx, score, k, lam)
    assert st == 0 and int(err.item()) == 1
    _same(outs, ref, k, bad_value)
    st, outs, err = _raw(dim, _lists(dim, n_cand)[0], score, k, lam)         # and the flag is cleared by a clean call
    assert st == 0 and int(err.item()) == 0


def test_einval_returns_before_writing():
    import torch
    dim, n_cand, k, lam = 128, 20, 5, 0.5
    idx, score = _lists(dim, n_cand)
    cases = [dict(dim_arg=48), dict(dim_arg=0), dict(n_rows=0), dict(n_lists=-1), dict(n_cand=-1), dict(k=0), dict(k=21),
             dict(n_cand=257, k=5), dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan"))]
    cases += [dict(null=n) for n in ("What", "cand_idx", "cand_score", "out_idx", "out_pos", "out_score", "out_pen", "err")]

    def untouched(tensors):
        return all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in tensors)

    for kw in cases:
        st, outs, err = _raw(dim, idx, score, **dict(dict(k=k, lam=lam), **kw))
        assert st == -1 and untouched(outs + [err]), kw
    st, outs, err = _raw(dim, idx, score, k, lam, n_lists=0)                 # no lists: ok, nothing enqueued
    assert st == 0 and untouched(outs + [err])


def test_the_call_is_graph_capturable():
    """captured into a graph the call runs nothing; the replay writes the restatement's bits and clears the flag"""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    dim, n_cand, k, lam = 128, 100, 10, 0.3
    Wh = _table(dim)[0]
    idx, score = _lists(dim, n_cand)
    ci, cs = _cuda(idx), _cuda(score)
    outs = [poison.fill(torch.empty((N_LISTS, k), dtype=dt, device="cuda"), 0x3F)
            for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x3F)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = lib.anirec_mmr_rerank(_lib.ptr(Wh), dim, N_ROWS, _lib.ptr(ci), _lib.ptr(cs), N_LISTS, n_cand, k, lam,
                                   *[_lib.ptr(o) for o in outs], _lib.ptr(err),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    assert all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in outs + [err])     # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    _same(outs, _reference(dim, n_cand, lam), k, "graph replay")


def test_lam_one_on_the_pool_is_predict_topk():
    """lam = 1 on predict_topk(pool) candidates: predict_topk(k), bit for bit"""
    import torch
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(8)
    dim, n_a, pool, k = 64, 400, 100, 10
    U = _cuda(rng.normal(size=(60, dim)).astype(np.float32))
    A = _cuda(rng.normal(size=(n_a, dim)).astype(np.float32))
    head = dict(w=1.3, b=-0.1, gamma=0.9, beta=0.05, mov_mean=0.02, mov_var=0.8)
    users = np.arange(N_LISTS)
    cand, p = ops.predict_topk(U, A, head, users, pool)
    want_i, want_p = ops.predict_topk(U, A, head, users, k)
    gi, gpos, gs, _ = ops.mmr_rerank(ops.rownorm(A), cand, p, k, 1.0)
    assert torch.equal(gi, want_i) and torch.equal(gs.view(torch.int32), want_p.view(torch.int32))
    assert torch.equal(gpos, torch.arange(k, dtype=torch.int32, device="cuda").expand(N_LISTS, k))


def test_planted_franchises_are_spread():
    """12 clusters of 8 rows around distinct basis vectors: lam = 0.5, k = 12 picks one anime of every cluster, the plain
    top-12 repeats clusters.  With within-cluster cosines >= 0.95 and between-cluster cosines <= 0.2 (asserted from the
    input) a candidate of a cluster already picked has val <= 0.5 * 1 - 0.5 * 0.95 = 0.025 and one of a fresh cluster
    val >= 0.5 * 0.5 - 0.5 * 0.2 = 0.15: the score spread (0.5) is smaller than the penalty gap (0.75)."""
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(0)
    dim, n_cl, per = 32, 12, 8
    W = np.repeat(np.eye(dim, dtype=np.float32)[:n_cl], per, axis=0) + rng.normal(0, 0.02, (n_cl * per, dim)).astype(np.float32)
    cluster = np.repeat(np.arange(n_cl), per)
    Wn = W.astype(np.float64) / np.linalg.norm(W.astype(np.float64), axis=1, keepdims=True)
    C = Wn @ Wn.T
    same = cluster[:, None] == cluster[None, :]
    print("within-cluster cosine >= %.3f, between-cluster <= %.3f" % (C[same].min(), C[~same].max()))
    assert C[same].min() >= 0.95 and C[~same].max() <= 0.2
    order = rng.permutation(n_cl * per).astype(np.int32)
    score = np.sort(rng.uniform(0.5, 1.0, n_cl * per).astype(np.float32))[::-1].copy()
    assert len(set(cluster[order[:n_cl]].tolist())) < n_cl                  # the plain top-12 repeats clusters
    gi, gpos, gs, gpen = ops.mmr_rerank(ops.rownorm(_cuda(W)), _cuda(order[None]), _cuda(score[None]), n_cl, 0.5)
    picked = gi.cpu().numpy()[0]
    assert sorted(cluster[picked].tolist()) == list(range(n_cl))            # every pick from a fresh cluster
    assert gpos.cpu().numpy()[0, 0] == 0 and float(gpen.cpu().numpy()[0].max()) <= 0.2 + 1e-6


# ---- recs.diverse_topk and the component, on the pipeline of test_components_gpu.py --------------------------------
def _model():
    from anime_recommendations_amd import artifacts, weights_io
    return weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest"))


def test_diverse_topk_on_the_trained_model(pipeline):  # noqa: F811
    import torch
    from anime_recommendations_amd import ops, recs, weights_io
    m = _model()
    U, A, head = _cuda(np.asarray(m["U"], np.float32)), _cuda(np.asarray(m["A"], np.float32)), weights_io.model_head(m)
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    users = np.array([3, 50, 120, 299])
    uid, aid = np.asarray(m["user_ids"]), np.asarray(m["anime_ids"])
    mine = df[df.user_id.isin(uid[users])]
    u_pos = pd.Index(uid[users]).get_indexer(mine.user_id)
    a_pos = pd.Index(aid).get_indexer(mine.anime_id)
    assert (u_pos >= 0).all() and (a_pos >= 0).all()
    watched = ops.seen_bits(u_pos.astype(np.int32), a_pos.astype(np.int32), len(users), len(aid))
    k, pool = 10, 100
    # diversity 0: ops.predict_topk itself
    gi, gp, gpen = recs.diverse_topk(U, A, head, users, k, pool, 0.0, watched)
    wi, wp = ops.predict_topk(U, A, head, users, k, watched)
    assert gpen is None and torch.equal(gi, wi) and torch.equal(gp.view(torch.int32), wp.view(torch.int32))
    # diversity 0.3: the restatement on (the pool list, cosine_scores), several users at once, under the watched mask
    gi, gp, gpen = recs.diverse_topk(U, A, head, users, k, pool, 0.3, watched)
    cand, p = ops.predict_topk(U, A, head, users, pool, watched)
    Wh = ops.rownorm(A)
    S = np.stack([ops.cosine_scores(Wh, q).cpu().numpy() for q in range(len(aid))])
    ri, _, rs, rn = M.rerank_lists(S, Wh.cpu().numpy(), cand.cpu().numpy(), p.cpu().numpy(), k, 1 - 0.3)
    assert np.array_equal(gi.cpu().numpy(), ri) and np.array_equal(_bits(gp.cpu().numpy()), _bits(rs))
    assert np.array_equal(_bits(gpen.cpu().numpy()), _bits(rn))
    for r in range(len(users)):                                 # nothing watched is listed
        assert not (set(aid[gi.cpu().numpy()[r]].tolist()) & set(df[df.user_id == uid[users[r]]].anime_id))
    # a pool beyond the table is clamped to it
    ci, cp, _ = recs.diverse_topk(U[:, :32].contiguous(), A[:, :32].contiguous(), head, users, k, 10 ** 6, 0.3)
    assert tuple(ci.shape) == (len(users), k) and bool((ci >= 0).all())


def test_diverse_recs_component(pipeline, golden_dir):  # noqa: F811
    from anime_recommendations_amd import components as C, weights_io
    work, env = pipeline["work"], pipeline["env"]
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    user = int(df.user_id.unique()[5])
    m = _model()
    anime_df = C.load_anime_df(pipeline["paths"]["all_anime"])
    syn_df = C.load_synopses(pipeline["paths"]["synopses"])
    user_ids, anime_ids = C.index_tables(m, df)
    fmt = json.load(open(os.path.join(golden_dir, "reference_output_formats.json")))["User_ID_153695_model_recs.csv"]
    frames = {}
    for diversity in (0.3, 0):
        flags = dict(main_df="user_stats.parquet:latest", main_df_type="parquet", project_name="anime_recommendations",
                     anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopsis_df="synopses.csv:latest",
                     sypnopsis_df_type="raw_data", model="wandb_anime_nn.h5:latest", model_type="h5",
                     model_user_query=user, random_user=False, model_recs_fn="model_recs.csv", save_model_recs=True,
                     model_num_recs=10, anime_types='["TV", "Movie"]', specify_types=True,
                     model_genres='["Action", "Comedy", None]', specify_genres=False, model_ID_flow=False,
                     model_ID_conf=True, model_recs_type="csv", flow_ID="user_id.csv:latest", flow_ID_type="csv",
                     diversity=diversity, pool=60)
        _run("diverse_recs", flags, str(work), env)
        got = pd.read_csv(work / ("User_ID_%d_diverse_model_recs.csv" % user))
        assert got.columns.tolist() == fmt["columns"] + ["Max_similarity"] and len(got) == fmt["n_rows"]
        want, stats = C.diverse_recs_frame(m["U"], m["A"], weights_io.model_head(m), user_ids, anime_ids, df, anime_df,
                                           syn_df, user, 10, types=["TV", "Movie"], pool=60, diversity=diversity)
        assert got["anime_id"].tolist() == want["anime_id"].tolist() and got["Name"].tolist() == want["Name"].tolist()
        for col in ("Prediction", "Max_similarity"):
            assert np.array_equal(got[col].to_numpy().astype(np.float32), want[col].to_numpy().astype(np.float32)), col
        assert got["Type"].isin(["TV", "Movie"]).all() and not (set(got["anime_id"]) & set(df[df.user_id == user].anime_id))
        assert got["Max_similarity"].iloc[0] == 0 and np.isfinite(list(stats.values())).all()
        frames[diversity] = (got, stats)
    plain = C.model_recs_frame(m["U"], m["A"], weights_io.model_head(m), user_ids, anime_ids, df, anime_df, syn_df, user,
                               10, types=["TV", "Movie"])
    got0, stats0 = frames[0]
    assert got0["anime_id"].tolist() == plain["anime_id"].tolist()
    assert np.array_equal(got0["Prediction"].to_numpy().astype(np.float32), plain["Prediction"].to_numpy())
    assert stats0["mean_similarity"] == stats0["mean_similarity_topk"]
    assert frames[0.3][1]["mean_similarity_topk"] == pytest.approx(stats0["mean_similarity"], abs=1e-12)
