"""GPU tests of the list evaluation (anirec_list_similarity, ops.list_similarity, recs.list_quality,
components.evaluate_lists_frame, the evaluate component's lists leg).

Yardstick: the NumPy restatement (tests/listeval_restatement.py) run on the similarities the existing
``ops.cosine_scores`` returns for the same normalised table — that kernel is not under test here, and the header defines
sim(s, j) as its chain, bit for bit.  Every comparison of the sim_max and sim_sum bits is exact, NaNs included.

Shapes: test_mmr_gpu's 777-row tables (widths 32, 64, 128, 256, with two bit-identical rows and a zero row), 37 lists a
call, the first of them with the content ``_lists`` plants; k 1, 2, 10, 63, 64, 65 (a wave and one past it) and
anirec_mmr_max_cand(width) (the full LDS image, row blocks of 4 .. 32 rows), and 15, 16, 25, 26, 32, 33: the list
lengths either side of the wave-per-list / workgroup-per-list switch at widths 256, 128 and 64 / 32.
"""
import ctypes
import json
import os

import numpy as np
import pandas as pd
import pytest

import listeval_restatement as L
import poison
from test_components_gpu import _run, pipeline  # noqa: F401  (the components' pipeline fixture, as it is)
from test_mmr_gpu import N_LISTS, N_ROWS, TWIN_A, TWIN_B, WIDTHS, ZERO_ROW, _bits, _cuda, _table
from test_mmr_gpu import _lists as _mmr_lists

pytestmark = pytest.mark.gpu
KS = (1, 2, 10, 15, 16, 25, 26, 32, 33, 63, 64, 65, "max")


def _k(dim, k):
    from anime_recommendations_amd import _lib
    return _lib.mmr_max_cand(dim) if k == "max" else k


def _lists(dim, k, seed=0):
    """N_LISTS lists of k random rows, the first ones with the content that takes a path of its own, as far as k has room
    for it"""
    rng = np.random.default_rng(seed * 1000 + dim + k)
    idx = rng.integers(0, N_ROWS, (N_LISTS, k)).astype(np.int32)
    idx[idx == ZERO_ROW] = ZERO_ROW + 1
    mid = k // 2
    idx[0, [0, mid, k - 1]] = -1                                # empty slots at the front, the middle and the end
    idx[1, :] = -1                                              # an all-empty list
    idx[2, :] = -1
    idx[2, mid] = 3                                             # one present slot
    idx[5, 0] = ZERO_ROW                                        # a zero row (NaN once normalised) first ...
    idx[6, k - 1] = ZERO_ROW                                    # ... and last
    if k >= 2:
        idx[3, 1] = idx[3, 0]                                   # a repeated index: two slots
        idx[4, 0], idx[4, k - 1] = TWIN_B, TWIN_A               # two bit-identical table rows
    if k >= 3:
        idx[7, mid] = ZERO_ROW
    return idx


_REFS = {}


def _reference(dim, k, seed=0):
    key = (dim, k, seed)
    if key not in _REFS:
        _REFS[key] = L.similarity_lists(_table(dim)[2], _lists(dim, k, seed))
    return _REFS[key]


def _same(got, ref, what):
    gm, gs = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in got]
    assert np.array_equal(_bits(gm), _bits(ref[0])), what
    assert np.array_equal(_bits(gs), _bits(ref[1])), what


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_similarity_equals_the_restatement(dim, k):
    from anime_recommendations_amd import ops
    k = _k(dim, k)
    Wh, _, S = _table(dim)
    idx = _lists(dim, k)
    ref = _reference(dim, k)
    _same(ops.list_similarity(Wh, _cuda(idx)), ref, (dim, k))
    # the planted content did what it is there for (checked on the reference, which the kernel has just equalled)
    rm, rs = ref
    nan = np.uint32(0x7FC00000)
    assert (_bits(rm[1]) == nan).all() and (_bits(rs[1]) == nan).all()
    assert rm[2, k // 2] == 0 and rs[2, k // 2] == 0 and np.isnan(np.delete(rs[2], k // 2)).all()
    assert (_bits(rm[0, [0, k // 2, k - 1]]) == nan).all()
    assert rm[5, 0] == 0 and rs[5, 0] == 0 and np.isnan(rm[5, 1:]).all() and np.isnan(rs[5, 1:]).all()
    if k >= 2:
        assert np.isnan(rs[6, k - 1]) and np.isfinite(rs[6, :k - 1]).all()
        assert _bits(rm[3, 1]) == _bits(S[idx[3, 0], idx[3, 0]]) and rm[3, 1] > 0.999
        assert _bits(rm[4, k - 1]) == _bits(S[TWIN_A, TWIN_B]) and rm[4, k - 1] > 0.999
    if k >= 3:
        assert np.isfinite(rs[7, :k // 2]).all() and np.isnan(rs[7, k // 2:]).all()
    if k >= 4:
        assert np.isfinite(rm[0, 1:k // 2]).all() and rm[0, 1] == 0         # the first PRESENT slot is slot 1


@pytest.mark.parametrize("n_cand,k", [(100, 10), (10, 10)])
def test_sim_max_is_the_rerank_pen(n_cand, k):
    """ops.list_similarity on anirec_mmr_rerank's out_idx: sim_max has that call's out_pen bits, padding included —
    at k < n_cand, and for a call whose lists run out of candidates (-1 / NaN tails)"""
    from anime_recommendations_amd import ops
    for dim in (64, 128):
        Wh = _table(dim)[0]
        idx, score = _mmr_lists(dim, n_cand)
        out_idx, _, _, out_pen = ops.mmr_rerank(Wh, _cuda(idx), _cuda(score), k, 0.3)
        sim_max, sim_sum = ops.list_similarity(Wh, out_idx)
        assert np.array_equal(_bits(sim_max.cpu().numpy()), _bits(out_pen.cpu().numpy()))
        pad = out_idx.cpu().numpy() < 0                         # (the lists with one present candidate, or none)
        assert pad.any() and np.isnan(sim_sum.cpu().numpy()[pad]).all()
        assert (pad.sum(axis=1) > 0).sum() > (3 if n_cand == k else 1)      # n_cand == k: every list with a -1 runs out


def test_a_list_does_not_depend_on_its_context():
    """a list run alone, at another position among other lists, and twice: the same bits — for a wave-per-list and a
    workgroup-per-list shape"""
    from anime_recommendations_amd import ops
    for dim, k in ((128, 10), (128, 100)):
        Wh = _table(dim)[0]
        idx = _lists(dim, k)
        ref = _reference(dim, k)
        ci = _cuda(idx)
        _same(ops.list_similarity(Wh, ci), ref, "whole call")
        _same(ops.list_similarity(Wh, ci), ref, "second run")
        perm = np.random.default_rng(5).permutation(N_LISTS)
        _same(ops.list_similarity(Wh, _cuda(idx[perm])), [r[perm] for r in ref], "permuted call")
        for l in (0, 7, 20, 36):
            _same(ops.list_similarity(Wh, ci[l:l + 1].clone()), [r[l:l + 1] for r in ref], "list %d alone" % l)


@pytest.mark.parametrize("byte", poison.ORDER)
def test_dirty_outputs_are_fully_overwritten(byte):
    from anime_recommendations_amd import ops
    for dim, k in ((32, 65), (128, 10), (256, 128)):
        Wh = _table(dim)[0]
        ci = _cuda(_lists(dim, k))
        log = []
        with poison.poisoned(byte, log):
            got = ops.list_similarity(Wh, ci)
        assert len(log) == 3 and sum(log) == 2 * N_LISTS * k * 4 + 4        # the two outputs and the flag word
        _same(got, _reference(dim, k), (byte, dim))


def _raw(dim, idx, k=None, n_rows=N_ROWS, n_lists=None, null=None, fill=0x3F, dim_arg=None):
    """anirec_list_similarity itself, its outputs and flag pre-filled with ``fill`` bytes: no wrapper check between the
    test and the entry point.  ``null``: the name of one pointer passed as NULL.  Returns (status, outs, err)."""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    k = idx.shape[1] if k is None else k
    shape = (idx.shape[0], max(k, idx.shape[1]))
    outs = [poison.fill(torch.empty(shape, dtype=torch.float32, device="cuda"), fill) for _ in range(2)]
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), fill)
    p = dict(What=_table(dim)[0], list_idx=_cuda(idx), out_max=outs[0], out_sum=outs[1], err=err)
    if null:
        p[null] = None
    st = lib.anirec_list_similarity(_lib.ptr(p["What"]), dim if dim_arg is None else dim_arg, n_rows,
                                    _lib.ptr(p["list_idx"]), idx.shape[0] if n_lists is None else n_lists, k,
                                    _lib.ptr(p["out_max"]), _lib.ptr(p["out_sum"]), _lib.ptr(p["err"]),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, outs, err


@pytest.mark.parametrize("bad_value", [N_ROWS, -2, 2 ** 31 - 1])
def test_a_bad_index_poisons_its_own_list_alone(bad_value):
    from anime_recommendations_amd import ops
    for dim, k, l in ((64, 10, 21), (64, 65, 20)):              # (list 21 shares its workgroup with 20, 22 and 23)
        idx = _lists(dim, k).copy()
        ref = [r.copy() for r in _reference(dim, k)]
        idx[l, k - 1] = bad_value
        ref[0][l], ref[1][l] = np.nan, np.nan
        st, outs, err = _raw(dim, idx)
        assert st == 0 and int(err.item()) == 1
        _same(outs, ref, (bad_value, k))
        with pytest.raises(ValueError, match="out of range"):
            ops.list_similarity(_table(dim)[0], _cuda(idx))
        st, outs, err = _raw(dim, _lists(dim, k))                # and the flag is cleared by a clean call
        assert st == 0 and int(err.item()) == 0
        _same(outs, _reference(dim, k), "clean")


def test_einval_returns_before_writing():
    import torch
    dim, k = 128, 20
    idx = _lists(dim, k)
    cases = [dict(dim_arg=48), dict(dim_arg=0), dict(n_rows=0), dict(n_rows=-5), dict(n_lists=-1), dict(k=0), dict(k=-1),
             dict(k=257)]
    cases += [dict(null=n) for n in ("What", "list_idx", "out_max", "out_sum", "err")]

    def untouched(tensors):
        return all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in tensors)

    for kw in cases:
        st, outs, err = _raw(dim, idx, **kw)
        assert st == -1 and untouched(outs + [err]), kw
    st, outs, err = _raw(dim, idx, n_lists=0)                   # no lists: ok, nothing enqueued
    assert st == 0 and untouched(outs + [err])


def test_the_call_is_graph_capturable():
    """captured into a graph the call runs nothing; the replay writes the restatement's bits and clears the flag"""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    for dim, k in ((128, 10), (128, 100)):
        Wh = _table(dim)[0]
        ci = _cuda(_lists(dim, k))
        outs = [poison.fill(torch.empty((N_LISTS, k), dtype=torch.float32, device="cuda"), 0x3F) for _ in range(2)]
        err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x3F)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            st = lib.anirec_list_similarity(_lib.ptr(Wh), dim, N_ROWS, _lib.ptr(ci), N_LISTS, k, _lib.ptr(outs[0]),
                                            _lib.ptr(outs[1]), _lib.ptr(err),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        torch.cuda.synchronize()
        assert all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in outs + [err])     # captured, not run
        graph.replay()
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        _same(outs, _reference(dim, k), "graph replay")


def test_list_quality_equals_the_figures_of_the_restatement():
    """recs.list_quality (kernel + torch on the device) against recs.list_figures fed the restatement's similarities on
    the host: the same float64 figures (sums of the same fp32 values; torch's reduction order differs between devices, so
    to a few ulps), over the first k columns of wider lists"""
    import torch
    from anime_recommendations_amd import recs
    dim, k = 64, 10
    Wh = _table(dim)[0]
    idx = _lists(dim, 16)
    idx[idx == ZERO_ROW] = -1                                   # (finite figures: the NaN rows are covered above)
    rng = np.random.default_rng(3)
    row, anime = rng.integers(0, N_LISTS, 200), rng.integers(0, N_ROWS, 200)
    row[:37], anime[:37] = np.arange(N_LISTS), idx[:, 4]        # found ones among them (list 1 and 2 hold -1 there)
    anime[anime < 0] = 0
    count = rng.integers(0, 50, N_ROWS).astype(np.float32)
    got = recs.list_quality(Wh, _cuda(idx), k, row, anime, item_count=_cuda(count), n_raters=50)
    mx, sm = L.similarity_lists(_table(dim)[2], idx[:, :k])
    want = recs.list_figures(torch.from_numpy(idx[:, :k].copy()), N_ROWS, torch.from_numpy(mx), torch.from_numpy(sm), row,
                             anime, item_count=count, n_raters=50)
    assert sorted(got) == sorted(want) and got["n_lists"] == N_LISTS and got["n_targets"] == 200
    assert got["hit_rate"] >= 34 / 200
    for key in want:
        assert got[key] == pytest.approx(want[key], rel=1e-13, abs=0), key


# ---- two independent routes to the hits ------------------------------------------------------------------------------
HEAD = dict(w=1.3, b=-0.1, gamma=0.9, beta=0.05, mov_mean=0.02, mov_var=0.8)


def _small_model():
    """60 users x 400 anime at width 64 and 3000 distinct (user, anime) ratings, the last 500 held out"""
    from anime_recommendations_amd import data
    rng = np.random.default_rng(21)
    n_users, n_anime, dim = 60, 400, 64
    U = rng.normal(size=(n_users, dim)).astype(np.float32)
    A = rng.normal(size=(n_anime, dim)).astype(np.float32)
    pair = rng.permutation(n_users * n_anime)[:3000]            # distinct pairs: no target is also a training rating
    table = data.RatingTable(pair // n_anime, pair % n_anime, rng.integers(0, 11, 3000) / 10.0,
                             np.arange(n_users) * 3 + 7, np.arange(n_anime) * 2 + 1)
    model = dict(U=U, A=A, head=HEAD, user_ids=table.user_ids, anime_ids=table.anime_ids, activation="sigmoid")
    return model, table


def test_list_hits_are_the_ranks_below_k():
    """the targets' positions in predict_topk(k) lists are exactly predict_rank's ranks where rank < k and missing
    elsewhere, so the diversity = 0 row of evaluate_lists_frame holds evaluate_frame's hit_rate@k and ndcg@k to the bit"""
    from anime_recommendations_amd import components as C, ops, recs
    model, table = _small_model()
    k = 10
    users, row, anime, train = C.held_out_targets(table, 500, 0.5)
    assert len(row) > 150
    tU, tA = _cuda(model["U"]), _cuda(model["A"])
    seen = recs.listed_seen_bits(table.user[train], table.anime[train], users, table.n_users, table.n_anime)
    rank, _ = ops.predict_rank(tU, tA, HEAD, users, row, anime, watched_bits=seen)
    rank = rank.cpu().numpy().astype(np.int64)
    lists, _ = ops.predict_topk(tU, tA, HEAD, users, k, seen)
    pos = recs.hit_positions(lists, row, anime)
    assert (rank < k).sum() >= 1 and (rank >= k).sum() >= 100          # both kinds among the targets
    assert np.array_equal(pos, np.where(rank < k, rank, -1))
    frame, summary = C.evaluate_frame(model, table, 500, [1, k], 0.5)
    lf, ls = C.evaluate_lists_frame(model, table, 500, 0.5, [0, 0.4], k=k, pool=50)
    assert lf.columns.tolist() == C.LISTS_COLUMNS and lf["diversity"].tolist() == [0.0, 0.4]
    assert lf["hit_rate"][0] == summary["hit_rate@%d" % k] == ls["lists_hit_rate@0"]
    assert lf["ndcg"][0] == summary["ndcg@%d" % k] == ls["lists_ndcg@0"]
    assert 0 < lf["mrr"][0] <= summary["mrr"]                   # (the whole-ranking mrr also counts the ranks past k)
    assert np.isfinite(lf.to_numpy()).all()
    assert sorted(ls) == sorted("lists_%s@%s" % (c, d) for c in C.LISTS_COLUMNS[3:] for d in ("0", "0.4"))


def test_planted_franchises_are_spread():
    """test_mmr_gpu's cluster table — 12 clusters of 8 rows around distinct basis vectors, within-cluster cosines >= 0.95
    and between-cluster cosines <= 0.2, asserted from the input: the diversity 0.5 list takes one row of every cluster,
    so all its pairs are between clusters and mean_similarity <= 0.2; the plain top-12 repeats clusters, so it holds a
    pair >= 0.95 and its mean_max_similarity (from the input's float64 cosines: above 0.25) lies above 0.2, which bounds
    the re-ranked list's.  A cosine of the kernel is a 32-term fp32 chain of unit rows: within 32 * 2**-24 < 1e-5 of the
    float64 one, rownorm's own rounding included."""
    from anime_recommendations_amd import ops, recs
    rng = np.random.default_rng(0)
    dim, n_cl, per = 32, 12, 8
    W = np.repeat(np.eye(dim, dtype=np.float32)[:n_cl], per, axis=0) + rng.normal(0, 0.02, (n_cl * per, dim)).astype(np.float32)
    cluster = np.repeat(np.arange(n_cl), per)
    Wn = W.astype(np.float64) / np.linalg.norm(W.astype(np.float64), axis=1, keepdims=True)
    Cos = Wn @ Wn.T
    same = cluster[:, None] == cluster[None, :]
    print("within-cluster cosine >= %.3f, between-cluster <= %.3f" % (Cos[same].min(), Cos[~same].max()))
    assert Cos[same].min() >= 0.95 and Cos[~same].max() <= 0.2
    order = rng.permutation(n_cl * per).astype(np.int32)
    score = np.sort(rng.uniform(0.5, 1.0, n_cl * per).astype(np.float32))[::-1].copy()
    assert len(set(cluster[order[:n_cl]].tolist())) < n_cl                  # the plain top-12 repeats clusters
    top = order[:n_cl]
    plain_max = np.mean([Cos[top[s], top[:s]].max() for s in range(1, n_cl)])
    assert plain_max > 0.25
    Wh = ops.rownorm(_cuda(W))
    spread, _, _, _ = ops.mmr_rerank(Wh, _cuda(order[None]), _cuda(score[None]), n_cl, 0.5)
    plain = _cuda(order[None, :n_cl])
    q_spread, q_plain = recs.list_quality(Wh, spread), recs.list_quality(Wh, plain)
    print("diversity 0.5: %r\nplain top-12: %r" % (q_spread, q_plain))
    assert q_spread["mean_similarity"] <= 0.2
    assert abs(q_plain["mean_max_similarity"] - plain_max) < 1e-5
    assert q_plain["mean_max_similarity"] > 0.2 >= q_spread["mean_max_similarity"]
    assert float(ops.list_similarity(Wh, plain)[0].max()) >= 0.95 - 1e-5
    assert q_spread["coverage"] == q_plain["coverage"] == 12 / 96


# ---- the evaluate component's lists leg, on the pipeline of test_components_gpu.py -----------------------------------
def test_evaluate_component_lists_leg(pipeline):  # noqa: F811
    from anime_recommendations_amd import artifacts
    work, env = pipeline["work"], pipeline["env"]
    ks = [1, 10, 50]
    ev = dict(input_data="user_stats.parquet:latest", main_df_type="parquet", model="wandb_anime_nn.h5:latest",
              model_type="h5", project_name="anime_recommendations", test_size=2000, eval_k=str(ks), min_rating=0.7,
              eval_csv="ranking_metrics.csv", eval_type="eval_csv", ID_emb_name="user_embedding",
              anime_emb_name="anime_embedding")
    # without the flag: no lists file, and the printed summary's keys are the ranking ones alone
    plain = json.loads(_run("evaluate", ev, str(work), env).strip().splitlines()[-1])
    assert not os.path.exists(work / "eval_lists.csv")
    assert list(plain) == ["n", "n_users", "test_size", "min_rating", "mrr", "mean_rank", "median_rank"] + \
        [f % k for k in ks for f in ("hit_rate@%d", "ndcg@%d")]
    ranks = pd.read_csv(work / "ranking_metrics.csv", float_precision="round_trip")
    out = _run("evaluate", dict(ev, lists_diversity="[0, 0.3]", lists_pool=60), str(work), env)
    summary = json.loads(out.strip().splitlines()[-1])
    lists = pd.read_csv(work / "eval_lists.csv", float_precision="round_trip")
    assert lists.columns.tolist() == ["diversity", "k", "pool", "hit_rate", "ndcg", "mrr", "mean_similarity",
                                      "mean_max_similarity", "coverage", "gini", "novelty"]
    assert len(lists) == 2 and lists["diversity"].tolist() == [0.0, 0.3] and lists["k"].tolist() == [10, 10]
    assert lists["pool"].tolist() == [60, 60] and np.isfinite(lists.to_numpy()).all()
    assert lists["hit_rate"][0] == ranks["hit_rate"][ranks["k"] == 10].item() == plain["hit_rate@10"]
    assert lists["ndcg"][0] == ranks["ndcg"][ranks["k"] == 10].item()
    pd.testing.assert_frame_equal(pd.read_csv(work / "ranking_metrics.csv", float_precision="round_trip"), ranks)
    assert list(summary)[:len(plain)] == list(plain) and {k: summary[k] for k in plain} == plain
    assert list(summary)[len(plain):] == ["lists_%s@%s" % (c, d) for d in ("0", "0.3") for c in lists.columns[3:]]
    assert summary["lists_mean_similarity@0.3"] == lists["mean_similarity"][1]
    logged = pd.read_csv(artifacts.use_artifact("eval_lists.csv:latest", "eval_csv"), float_precision="round_trip")
    pd.testing.assert_frame_equal(logged, lists)
