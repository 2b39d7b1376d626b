"""GPU tests of the learned hybrid weights (anirec_fuse_rank_grid; ops.fuse_rank_grid, recs.hybrid_rank_grid /
hybrid_fit_weights and evaluate --baseline hybrid_tuned).

Yardsticks: the NumPy restatement (tests/fuse_grid_restatement.py: one fusion per weight vector, then a count of order
values) and the library's own route, ``ops.rows_rank(ops.fuse_rows(w))`` per weight vector.  Every comparison is an
integer equality.

Shapes: row lengths around the chunk of four items a load holds (1, 2, 3), around the wave (63, 64, 65), past the
largest workgroup of the sort (1025) and the bound of the LDS image (20 480, two rows); grids around the 64 weight
vectors of a workgroup (1, 2, 63, 64, 65) and past two of them (130)."""
import ctypes
import json

import numpy as np
import pandas as pd
import pytest

import cooc_restatement as CR
import fuse_grid_restatement as G
import fuse_restatement as R
import poison
from test_cooc_gpu import fixture_store  # noqa: F401  (the recs fixture as an artifact store)
from test_fuse_gpu import ALS_PAR, KNN_PAR, _cuda, _masks, _members, _systems, recs_table  # noqa: F401
from test_rank_gpu import _run as _run_out

pytestmark = pytest.mark.gpu
N_ITEMS = (1, 2, 3, 63, 64, 65, 1025)
METHODS = ("rrf", "minmax")


def _targets(E, rng):
    """no target, one and several in turn over the rows that have an eligible item; shuffled"""
    tr, ta = [], []
    for i, r in enumerate(np.flatnonzero(E.any(axis=1))):
        el = np.flatnonzero(E[r])
        take = (1, 4, 0)[i % 3]
        pick = rng.choice(el, min(take, len(el)), replace=False)
        tr += [int(r)] * len(pick)
        ta += pick.tolist()
    order = rng.permutation(len(tr))
    return np.asarray(tr, np.int64)[order], np.asarray(ta, np.int64)[order]


def _grid(n_w, S, rng):
    """weight vectors with zeros, tiny and huge entries; vector 0 all ones"""
    g = rng.choice(np.float32([0, 0, 0.1, 0.5, 1, 1, 2.5, 1e-30, 3e38]), (n_w, S))
    g[0] = 1
    dead = ~(g > 0).any(axis=1)
    g[dead, rng.integers(0, S, int(dead.sum()))] = 1
    return g


def _check(dev, host, grid, method, c, n, tr, ta, bits=None, keep=None, library=True, what=None):
    """ops.fuse_rank_grid against the restatement and against rows_rank(fuse_rows(w)) per weight vector"""
    import torch
    from anime_recommendations_amd import ops
    wb = None if bits is None else _cuda(bits.view(np.int32))
    kp = None if keep is None else _cuda(keep)
    got = ops.fuse_rank_grid(dev, grid, method, c, tr, ta, n=n, wbits=wb, keep=kp)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (len(grid), len(tr)), what
    want, err = G.rank_grid(host, grid, R.METHODS[method], c, tr, ta, n, bits, keep)
    assert err == 0, what
    g = got.cpu().numpy()
    bad = np.argwhere(g != want)
    assert not len(bad), (what, len(bad), bad[:5].tolist(), g[g != want][:5].tolist(), want[g != want][:5].tolist())
    if library and len(tr):
        for w in range(len(grid)):
            fused = ops.fuse_rows(dev, grid[w].tolist(), method, c, n=n, wbits=wb, keep=kp)
            assert torch.equal(got[w], ops.rows_rank(fused, tr, ta, wb)), (what, "library", w)
    return got


# ---- the kernels against the restatement and the library's own route -------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", N_ITEMS)
def test_rank_grid_equals_the_restatement_and_the_library(n, method):
    rng = np.random.default_rng(1000 * n + len(method))
    # one system, one row, one weight vector, no masks, c = 0: every item a target
    for kind in ("normal", "four", "equal", "zeros", "special", "nan"):
        dev, host = _systems(1, n, [kind], rng)
        ta = rng.permutation(n)[:8]
        _check(dev, host, np.float32([[2.5]]), method, 0, n, np.zeros(len(ta), np.int64), ta, what=("solo", kind))
    # two systems, three rows: masks, a shared vector, ld > n with poison in the padding, a keep; 2 and 63 vectors.
    # (under a keep the library's route, whose rank knows no keep, counts a NaN it holds for an item that is not kept
    # above a target whose own fused value is NaN, which only "wide" rows under minmax produce: the restatement alone)
    for kinds, n_w in ((("normal", "four"), 2), (("special", "zeros"), 63), (("wide", "equal"), 2), (("nan", "normal"), 2)):
        dev, host = _systems(3, n, kinds, rng, shared=(1,), pad=(0,))
        W, bits, keep = _masks(3, n, rng)
        E = ~W & (keep != 0)[None]
        tr, ta = _targets(E, rng)
        _check(dev, host, _grid(n_w, 2, rng), method, 60, n, tr, ta, bits, keep,
               library=not (method == "minmax" and "wide" in kinds), what=("pair", kinds))
        tr, ta = _targets(~W, rng)
        _check(dev, host, _grid(2, 2, rng), method, 60, n, tr, ta, bits, what=("pair, no keep", kinds))
    # three systems over 67 rows; 64 and 65 vectors over three rows
    dev, host = _systems(67, n, ("normal", "special", "four"), rng, pad=(2,))
    W, bits, keep = _masks(67, n, rng)
    tr, ta = _targets(~W, rng)
    _check(dev, host, np.float32([[1, 0, 2.5], [1, 1, 1]]), method, 60, n, tr, ta, bits, what="67 rows")
    sel = tr < 3
    for n_w in (64, 65):
        _check([d[:3].contiguous() for d in dev], [h[:3] for h in host], _grid(n_w, 3, rng), method, 0, n, tr[sel], ta[sel],
               bits[:3], what=("three", n_w))
    # eight systems over three rows, 130 vectors
    dev, host = _systems(3, n, ("normal", "four", "equal", "zeros", "special", "nan", "wide", "normal"), rng, shared=(3,))
    tr, ta = _targets(np.ones((3, n), bool), rng)
    _check(dev, host, _grid(130, 8, rng), method, 0, n, tr, ta, library=False, what="eight")
    _check(dev, host, _grid(3, 8, rng), method, 60, n, tr, ta, what="eight, library")


def test_the_longest_rows():
    """the bound of the sort network and of the LDS image: two rows, three vectors"""
    n = 20480
    rng = np.random.default_rng(n)
    dev, host = _systems(2, n, ("special", "four"), rng, shared=(1,))
    W, bits, keep = _masks(2, n, rng)
    W[0] = rng.random(n) < 0.1
    bits = CR.pack_bits(W)
    tr, ta = _targets(~W & (keep != 0)[None], rng)
    tr, ta = np.concatenate([tr, [1, 0]]), np.concatenate([ta, [int(np.flatnonzero(~W[1] & (keep != 0))[-1]),
                                                                int(np.flatnonzero(~W[0] & (keep != 0))[-1])]])
    for method in METHODS:
        _check(dev, host, np.float32([[1, 1], [1, 0.5], [0, 1]]), method, 60, n, tr, ta, bits, keep, what=method)


def test_refusals_without_a_launch():
    import torch
    from anime_recommendations_amd import ops
    x = torch.zeros(2, 20481, dtype=torch.float32, device="cuda:0")
    small = x[:, :10].contiguous()
    with pytest.raises(ValueError, match="1 .. 20480"):
        ops.fuse_rank_grid([x], [[1.0]], "rrf", 60, [0], [0])
    with pytest.raises(ValueError, match="1 .. 4095"):
        ops.fuse_rank_grid([small], np.ones((4096, 1)), "rrf", 60, [0], [0])
    with pytest.raises(ValueError, match="same number of rows"):
        ops.fuse_rank_grid([small, torch.zeros(3, 10, device="cuda:0")], [[1, 1]], "rrf", 60, [0], [0])
    with pytest.raises(ValueError, match="one entry per target"):
        ops.fuse_rank_grid([small], [[1.0]], "rrf", 60, [0, 1], [0])
    assert tuple(ops.fuse_rank_grid([small], np.ones((5, 1)), "rrf", 60, [], []).shape) == (5, 0)
    with pytest.raises(ValueError, match="no rows"):
        ops.fuse_rank_grid([torch.zeros(0, 10, device="cuda:0")], [[1.0]], "rrf", 60, [0], [0])


# ---- the entry point itself: dirty memory, a graph, the error flag ---------------------------------------------------
class _Raw:
    """anirec_fuse_rank_grid on device tensors the test owns"""

    def __init__(self, dev, n, nq, bits, keep, grid, tr, ta):
        import torch
        from anime_recommendations_amd import _lib
        self.lib, self.ptr = _lib.load(), _lib.ptr
        self.dev, self.n, self.nq, self.S = dev, n, nq, len(dev)
        self.ptrs = (ctypes.c_void_p * self.S)(*[r.data_ptr() for r in dev])
        self.lds = (ctypes.c_int64 * self.S)(*[int(r.shape[1]) if r.dim() == 2 else 0 for r in dev])
        self.wb = None if bits is None else _cuda(bits.view(np.int32))
        self.kp = None if keep is None else _cuda(keep)
        self.wg = _cuda(np.ascontiguousarray(grid, np.float32))
        self.tr, self.ta = _cuda(np.asarray(tr, np.int32)), _cuda(np.asarray(ta, np.int32))
        self.n_w, self.n_t = len(grid), len(tr)
        self.out = torch.empty(self.n_w, self.n_t, dtype=torch.int32, device="cuda:0")
        self.err = torch.empty(1, dtype=torch.int32, device="cuda:0")
        need = max(self.lib.anirec_fuse_rank_grid_workspace_bytes(self.S, n, nq, m) for m in (0, 1))
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")

    def __call__(self, method, c, out=None):
        import torch
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        out = self.out if out is None else out
        return self.lib.anirec_fuse_rank_grid(self.ptrs, self.lds, self.S, self.n, self.nq, self.ptr(self.wb),
                                              self.ptr(self.kp), R.METHODS[method], c, self.ptr(self.wg), self.n_w,
                                              self.ptr(self.tr), self.ptr(self.ta), self.n_t, self.ptr(out),
                                              self.ptr(self.err), self.ptr(self.ws), self.ws.numel(), s)


@pytest.mark.parametrize("method", METHODS)
def test_dirty_workspace_output_and_flag(method):
    """what the workspace, the output and the flag held changes nothing: the four patterns, the same call each time"""
    import torch
    rng = np.random.default_rng(5)
    nq, n = 5, 1025
    dev, host = _systems(nq, n, ("normal", "special", "four"), rng, shared=(2,), pad=(1,))
    W, bits, keep = _masks(nq, n, rng)
    tr, ta = _targets(~W & (keep != 0)[None], rng)
    grid = _grid(70, 3, rng)
    want, err = G.rank_grid(host, grid, R.METHODS[method], 7, tr, ta, n, bits, keep)
    assert err == 0 and len(tr)
    raw = _Raw(dev, n, nq, bits, keep, grid, tr, ta)
    for byte in poison.ORDER:
        for t in (raw.ws, raw.out, raw.err):
            poison.fill(t, byte)
        assert raw(method, 7) == 0
        assert int(raw.err.item()) == 0 and np.array_equal(raw.out.cpu().numpy(), want), (method, byte)
    raw.ws = raw.ws[:raw.ws.numel() - 16]                        # too small a workspace: refused, nothing written
    poison.fill(raw.out, 0x3F)
    assert raw(method, 7) == -3                                  # ANIREC_EWORKSPACE
    assert bool((raw.out.view(torch.uint8) == 0x3F).all())


def test_rank_grid_replays_from_a_graph():
    import torch
    rng = np.random.default_rng(8)
    nq, n = 4, 1025
    dev, host = _systems(nq, n, ("normal", "four"), rng)
    W, bits, _ = _masks(nq, n, rng)
    tr, ta = _targets(~W, rng)
    grid = _grid(65, 2, rng)
    raw = _Raw(dev, n, nq, bits, None, grid, tr, ta)
    out = {m: torch.empty(len(grid), len(tr), dtype=torch.int32, device="cuda:0") for m in METHODS}
    assert raw("rrf", 60) == 0                                   # the eager call first: attributes set outside the capture
    torch.cuda.synchronize()
    for o in out.values():
        poison.fill(o, 0x3F)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = [raw(m, 60, out[m]) for m in METHODS]
    assert st == [0, 0]
    torch.cuda.synchronize()
    assert all(bool((o.view(torch.uint8) == 0x3F).all()) for o in out.values())      # captured, not run
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for m in METHODS:
            want, _ = G.rank_grid(host, grid, R.METHODS[m], 60, tr, ta, n, bits)
            assert np.array_equal(out[m].cpu().numpy(), want), ("replay", m)
            poison.fill(out[m], 0x7F)
        assert int(raw.err.item()) == 0


@pytest.mark.parametrize("method", METHODS)
def test_the_error_flag_and_where_minus_one_goes(method):
    rng = np.random.default_rng(11)
    nq, n = 3, 65
    dev, host = _systems(nq, n, ("normal", "four"), rng, shared=(1,))
    W = rng.random((nq, n)) < 0.3
    W[:, 0], W[:, 1] = False, True
    keep = np.ones(n, np.uint8)
    keep[2] = 0
    bits = CR.pack_bits(W)
    good = (np.asarray([0, 1, 2, 2], np.int64), np.asarray([0, 0, 0, int(np.flatnonzero(~W[2] & (keep != 0))[-1])], np.int64))
    grid = np.float32([[1, 1], [0.5, 0], [0, 3]])
    cases = {"clean": (good, grid),
             "its own watched bit": ((np.append(good[0], 1), np.append(good[1], 1)), grid),
             "not kept": ((np.append(good[0], 0), np.append(good[1], 2)), grid),
             "row below": ((np.append(good[0], -1), np.append(good[1], 0)), grid),
             "row above": ((np.append(good[0], nq), np.append(good[1], 0)), grid),
             "anime below": ((np.append(good[0], 0), np.append(good[1], -1)), grid),
             "anime above": ((np.append(good[0], 0), np.append(good[1], n)), grid),
             "anime far above": ((np.append(good[0], 0), np.append(good[1], 2 ** 31 - 1)), grid),
             "a negative weight": (good, np.float32([[1, 1], [0.5, -1], [0, 3]])),
             "a NaN weight": (good, np.float32([[1, 1], [np.nan, 1], [0, 3]])),
             "an infinite weight": (good, np.float32([[np.inf, 1], [0.5, 0], [0, 3]])),
             "all zero": (good, np.float32([[1, 1], [0.5, 0], [0, -0.0]]))}
    clean = None
    for name, ((tr, ta), g) in cases.items():
        want, err = G.rank_grid(host, g, R.METHODS[method], 60, tr, ta, n, bits, keep)
        assert err == (name != "clean"), name
        raw = _Raw(dev, n, nq, bits, keep, g, tr, ta)
        poison.fill(raw.out, 0x3F)
        assert raw(method, 60) == 0, name
        got = raw.out.cpu().numpy()
        assert int(raw.err.item()) == err and np.array_equal(got, want), (name, got.tolist(), want.tolist())
        if name == "clean":
            clean = got
            assert (got >= 0).all()
        elif len(tr) == 5:                                       # -1 for the bad target alone, under every vector
            assert (got[:, 4] == -1).all() and np.array_equal(got[:, :4], clean), name
        else:                                                    # -1 for the bad vector alone, for every target
            bad = [w for w in range(3) if not G.weight_ok(g[w])]
            assert len(bad) == 1 and (got[bad[0]] == -1).all(), name
            assert np.array_equal(np.delete(got, bad[0], axis=0), np.delete(clean, bad[0], axis=0)), name
    from anime_recommendations_amd import _lib, ops
    with pytest.raises(_lib.AnirecError, match="not eligible"):
        ops.fuse_rank_grid(dev, grid, method, 60, [1], [1], n=n, wbits=_cuda(bits.view(np.int32)), keep=_cuda(keep))


# ---- the host layers on the recs fixture ------------------------------------------------------------------------------
def test_hybrid_rank_grid_on_the_recs_fixture(recs_table):  # noqa: F811
    import torch
    from anime_recommendations_amd import recs
    model, table = recs_table
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    assert len(row) > 100
    members, seen = _members(model, table, users, train)
    names = ("model", "popularity", "itemknn", "als")
    sources = [members[m][0] for m in names]
    rows = [src(0, len(users)).cpu().numpy() if callable(src) else src.cpu().numpy() for src in sources]
    sb = seen.cpu().numpy().view(np.uint32)
    grid = recs.hybrid_weight_grid(4, 3)
    for method in METHODS:
        want, err = G.rank_grid(rows, grid, R.METHODS[method], 60, row, anime, table.n_anime, sb)
        assert err == 0
        for batch in (1, 5, len(users)):
            got = recs.hybrid_rank_grid(sources, seen, row, anime, grid, method, 60, batch=batch)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (method, batch)
        assert torch.equal(got[0], recs.hybrid_rank(sources, seen, row, anime, None, method, 60))   # row 0: the default
        sums, best = recs.hybrid_fit_weights(got, row, len(users), "ndcg@10", table.n_anime)
        ref = G.gain_sums(want, row, len(users), "ndcg@10", table.n_anime)
        assert np.array_equal(sums, ref) and best == G.best(ref, np.ones(len(users), bool))


def test_evaluate_baseline_hybrid_tuned_on_the_recs_fixture(fixture_store):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, data, ops, recs, weights_io
    work, env, pq = fixture_store["work"], fixture_store["env"], fixture_store["pq"]
    ks = [1, 5, 20]
    ev = dict(input_data="user_stats.parquet:latest", main_df_type="parquet", model="wandb_anime_nn.h5:latest",
              model_type="h5", project_name="anime_recommendations", test_size=1000, eval_k=str(ks), min_rating=0.7,
              eval_csv="tuned_metrics.csv", eval_type="eval_csv", ID_emb_name="user_embedding",
              anime_emb_name="anime_embedding", baseline="popularity,hybrid,hybrid_tuned", ci_replicates=200,
              hybrid_tune_metric="ndcg@5", hybrid_tune_folds=3, hybrid_tune_seed=4)
    ev.update({"itemknn_" + k: v for k, v in KNN_PAR.items()})
    ev.update({"als_" + k: v for k, v in ALS_PAR.items()})
    code, out = _run_out("evaluate", ev, str(work), env)
    assert code == 0, out[-3000:]
    summary = json.loads(out.strip().splitlines()[-1])
    frame = pd.read_csv(work / "tuned_metrics.csv", float_precision="round_trip")
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    table = data.load_user_stats(pq)
    # without the tuned system the frame and the summary are what they were
    base_frame, base = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline=("popularity", "hybrid"), ci_replicates=200,
                                        itemknn=KNN_PAR, als=ALS_PAR)
    assert frame[base_frame.columns.tolist()].to_csv(index=False) == base_frame.to_csv(index=False)
    assert {k: summary[k] for k in base} == base
    assert frame.columns.tolist()[:9] == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity", "hit_rate_hybrid",
                                          "ndcg_hybrid", "hit_rate_hybrid_tuned", "ndcg_hybrid_tuned"]
    # the tuned columns from the restatement's cross-fitted ranks of the members' own rows
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    members, seen = _members(model, table, users, train)
    names = ("model", "itemknn", "als")
    rows = [members[m][0](0, len(users)).cpu().numpy() for m in names]
    sb = seen.cpu().numpy().view(np.uint32)
    grid = G.weight_grid(3, 10)
    ranks, err = G.rank_grid(rows, grid, R.RRF, 60, row, anime, table.n_anime, sb)
    assert err == 0 and len(grid) == 67
    tuned, picks, best_all = G.tuned(ranks, row, len(users), "ndcg@5", table.n_anime, 3, 4)
    assert summary["hybrid_tuned_metric"] == "ndcg@5" and summary["hybrid_tuned_grid"] == 67
    assert summary["hybrid_tuned_fold_weights"] == [grid[i].astype(np.float64).tolist() for i in picks]
    assert summary["hybrid_tuned_weights"] == grid[best_all].astype(np.float64).tolist()
    b = recs.ranking_metrics(tuned, ks)
    assert frame["hit_rate_hybrid_tuned"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_hybrid_tuned"].tolist() == [b["ndcg"][k] for k in ks]
    assert summary["hybrid_tuned_mrr"] == b["mrr"] and summary["hybrid_tuned_mean_rank"] == b["mean_rank"]
    tU, tA = members["model"][1]
    rank = ops.predict_rank(tU, tA, weights_io.model_head(model), users, row, anime, watched_bits=seen)[0]
    pop_rank = ops.score_rank(members["popularity"][0], len(users), row, anime, watched_bits=seen)
    boot = recs.bootstrap_metrics({"model": rank, "popularity": pop_rank, "hybrid": ranks[0], "hybrid_tuned": tuned}, row,
                                  len(users), ks, 200, 0, 0.95, unit_key=users, n_rows=table.n_anime)
    for i, k in enumerate(ks):
        for metric in ("hit_rate", "ndcg"):
            name = "%s@%d" % (metric, k)
            fig, d = boot["figures"]["hybrid_tuned"][name], boot["diffs"]["hybrid_tuned"][name]
            assert frame["%s_hybrid_tuned_lo" % metric][i] == fig["lo"] and frame["%s_hybrid_tuned_hi" % metric][i] == fig["hi"]
            assert frame["%s_diff_hybrid_tuned" % metric][i] == d["diff"] and frame["%s_p_hybrid_tuned" % metric][i] == d["p"]
    for key in ("mrr", "mean_rank"):
        assert summary["hybrid_tuned_%s_lo" % key] == boot["figures"]["hybrid_tuned"][key]["lo"]
        assert summary["%s_diff_hybrid_tuned" % key] == boot["diffs"]["hybrid_tuned"][key]["diff"]
        assert summary["%s_p_hybrid_tuned" % key] == boot["diffs"]["hybrid_tuned"][key]["p"]
