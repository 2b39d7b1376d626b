"""GPU tests of EASE (anirec_spd_inverse, anirec_ease_weights, anirec_ease_scores; the ops / recs wrappers; the
ease_recs component, evaluate --baseline ease and ease as a hybrid_recs member).

Yardsticks: for the inverse a residual, max |A P - I| <= 8 max(numpy.linalg.inv's residual, n 2^-52) (the matrix cores'
order inside one instruction is not documented, so no bit comparison with NumPy is possible; its own bits must repeat
and ignore the workspace); for the weights one fp32 ulp around the rounding of NumPy's own -P_ij / P_jj; for the score
rows the bits of the NumPy restatement (tests/ease_restatement.py) given the kernel's W.

Shapes: matrix sizes 1, 2 and on both sides of one, two and three blocks of the inverse; score rows of 1, 31, 33, 257
and one column tile + 1 items; lists that are empty, of one entry, with a repeated item and longer than one entry tile."""
import ctypes
import functools

import numpy as np
import pytest

import cooc_restatement as CR
import ease_cases as EC
import ease_restatement as R
import poison
import recs_fixture as RF
from component_cli import load_component
from test_cooc_gpu import fixture_store  # noqa: F401  (the recs fixture as an artifact store)

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
PAD = 7.25      # what the padding of a pitched buffer holds before and after a call


def _cuda(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _u32(x):
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    return np.ascontiguousarray(a).view(np.uint32)


def _u64(x):
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    return np.ascontiguousarray(a).view(np.uint64)


def _lib():
    from anime_recommendations_amd import _lib as L
    return L


def _nb():
    return int(_lib().load().anirec_spd_inverse_block())


def _sizes(case):
    nb = _nb()
    return {"nb-1": nb - 1, "nb": nb, "nb+1": nb + 1, "2nb+1": 2 * nb + 1, "3nb+5": 3 * nb + 5}.get(case, case)


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inverse(A, ld=None, ws_byte=0x3F):
    """(P fp64 [n, ld] with the padding as the call left it, info) through the library call itself"""
    import torch
    L = _lib()
    n = len(A)
    ld = n if ld is None else ld
    buf = torch.full((n, ld), PAD, dtype=torch.float64, device="cuda")
    buf[:, :n] = _cuda(A)
    info = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x3F)
    ws = poison.fill(torch.empty(int(L.load().anirec_spd_inverse_workspace_bytes(n)), dtype=torch.uint8, device="cuda"),
                     ws_byte)
    L.call("anirec_spd_inverse", buf, ld, n, info, ws, ws.numel(), _stream())
    return buf.cpu().numpy(), int(info.item())


# ---- the inverse ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [1.0, 50.0])
@pytest.mark.parametrize("size", [1, 2, "nb-1", "nb", "nb+1", "2nb+1", "3nb+5"])
def test_spd_inverse_meets_the_residual_and_repeats_its_bits(size, reg):
    n = _sizes(size)
    A = EC.gram_case(n, reg)
    bound, ref = EC.residual_bound(A)
    P, info = _inverse(A)
    res = R.residual(A, P)
    print("n = %d reg = %g: residual %.3g, numpy's %.3g, bound %.3g" % (n, reg, res, ref, bound))
    assert info == 0
    assert res <= bound
    again, info2 = _inverse(A)
    assert info2 == 0 and np.array_equal(_u64(again), _u64(P))
    for byte in (0xFF, 0x00):
        dirty, info3 = _inverse(A, ws_byte=byte)
        assert info3 == 0 and np.array_equal(_u64(dirty), _u64(P)), hex(byte)
    # the restatement, another summation order of the same algorithm, meets the same bound
    assert R.residual(A, R.spd_inverse(A, _nb())[0]) <= bound


def test_spd_inverse_leaves_the_padding_of_a_pitched_matrix_alone():
    from anime_recommendations_amd import ops
    n = _sizes("2nb+1")
    A = EC.gram_case(n, 50.0)
    P, info = _inverse(A, ld=n + 7)
    assert info == 0 and (P[:, n:] == PAD).all()
    dense, _ = _inverse(A)
    assert np.array_equal(_u64(P[:, :n]), _u64(dense))
    bound, _ = EC.residual_bound(A)
    assert R.residual(A, P[:, :n]) <= bound
    got, flag = ops.spd_inverse(_cuda(A))                               # the wrapper: the same bits, A kept
    assert int(flag.item()) == 0 and np.array_equal(_u64(got), _u64(dense))


def test_spd_inverse_reports_a_matrix_that_is_not_positive_definite():
    n = _sizes("nb+1")
    _, info = _inverse(-np.eye(n))
    assert info == 1
    A = EC.gram_case(n, 1.0)
    A[n - 1, n - 1] = -1e9                                              # the second block step's pivot
    _, info = _inverse(A)
    assert info == 2


# ---- the weights ------------------------------------------------------------------------------------------------------
def _ordered(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


@pytest.mark.parametrize("reg", [1.0, 50.0])
@pytest.mark.parametrize("size", [1, 2, "nb+1", "3nb+5"])
def test_ease_weights_are_within_an_ulp_of_numpy(size, reg):
    from anime_recommendations_amd import ops
    n = _sizes(size)
    A = EC.gram_case(n, reg)
    P, flag = ops.spd_inverse(_cuda(A))
    W = ops.ease_weights(P).cpu().numpy()
    want = R.ease_weights(np.linalg.inv(A))
    assert int(flag.item()) == 0 and W.shape == (n, n)
    d = np.abs(_ordered(W) - _ordered(want))
    print("n = %d reg = %g: %d of %d elements one ulp off, the largest distance %d" % (n, reg, int((d == 1).sum()), n * n,
                                                                                    int(d.max())))
    assert d.max() <= 1
    assert not _u32(W)[np.diag_indices(n)].any()                        # +0.0f, not -0.0f
    # the kernel's own rule on its own inverse: exact
    assert np.array_equal(_u32(W), _u32(R.ease_weights(P.cpu().numpy())))


def test_ease_weights_leave_the_padding_alone():
    import torch
    n = 33
    P = np.linalg.inv(EC.gram_case(n, 50.0))
    Pd = torch.full((n, n + 3), PAD, dtype=torch.float64, device="cuda")
    Pd[:, :n] = _cuda(P)
    W = torch.full((n, n + 5), PAD, dtype=torch.float32, device="cuda")
    _lib().call("anirec_ease_weights", Pd, n + 3, n, W, n + 5, _stream())
    W = W.cpu().numpy()
    assert (W[:, n:] == PAD).all() and np.array_equal(_u32(W[:, :n]), _u32(R.ease_weights(P)))


# ---- the score rows ---------------------------------------------------------------------------------------------------
def _col_tile():
    return int(_lib().load().anirec_ease_scores_col_tile())


def _entry_tile():
    return int(_lib().load().anirec_ease_scores_entry_tile())


@functools.lru_cache(maxsize=None)
def _weights(n):
    """The kernel's own W of a random case of n items, on the device and on the host"""
    from anime_recommendations_amd import ops
    P, flag = ops.spd_inverse(_cuda(EC.gram_case(n, 50.0)))
    assert int(flag.item()) == 0
    W = ops.ease_weights(P)
    return W, W.cpu().numpy()


N_LISTS = 12


@pytest.mark.parametrize("weights", [None, "positive", "signed"])
@pytest.mark.parametrize("size", [1, 31, 33, 257, "tile+1"])
def test_scores_equal_the_restatement(size, weights):
    from anime_recommendations_amd import ops
    n = _col_tile() + 1 if size == "tile+1" else size
    Wd, W = _weights(n)
    off, hist, hw = EC.score_lists(n, N_LISTS, 50 + n, _entry_tile() + 88, weights)
    assert off[4] - off[3] > _entry_tile()
    want, err = R.ease_scores(W, off, hist, hw)
    assert err == 0 and want.shape == (N_LISTS, n)
    got = ops.ease_scores(Wd, off, hist, hw)
    assert np.array_equal(_u32(got), _u32(want))
    assert not _u32(got)[0].any()                                       # no history: +0 everywhere
    for l in (0, 1, 2, 3, 7):                                           # a list alone is its row among the others
        w1 = None if hw is None else hw[off[l]:off[l + 1]]
        alone = ops.ease_scores(Wd, [0, off[l + 1] - off[l]], hist[off[l]:off[l + 1]], w1)
        assert alone.shape == (1, n) and np.array_equal(_u32(alone)[0], _u32(want)[l]), l
    perm = np.random.default_rng(1).permutation(int(off[4] - off[3])) + off[3]          # entry order changes nothing
    again = ops.ease_scores(Wd, [0, len(perm)], hist[perm], None if hw is None else hw[perm])
    assert np.array_equal(_u32(again)[0], _u32(want)[3])
    assert ops.ease_scores(Wd, [0], hist, hw).shape == (0, n)                           # no list


def test_scores_with_pitched_rows():
    import torch
    n = 257
    _, W = _weights(n)
    off, hist, hw = EC.score_lists(n, N_LISTS, 9, 40, "signed")
    want, _ = R.ease_scores(W, off, hist, hw)
    Wp = torch.full((n, n + 3), PAD, dtype=torch.float32, device="cuda")
    Wp[:, :n] = _cuda(W)
    out = torch.full((N_LISTS, n + 6), PAD, dtype=torch.float32, device="cuda")
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x3F)
    _lib().call("anirec_ease_scores", Wp, n + 3, n, _cuda(off), _cuda(hist), _cuda(hw), N_LISTS, len(hist), out, n + 6,
                err, _stream())
    out = out.cpu().numpy()
    assert int(err.item()) == 0 and (out[:, n:] == PAD).all() and np.array_equal(_u32(out[:, :n]), _u32(want))


def test_bad_values_raise_the_flag_and_spare_the_rest():
    from anime_recommendations_amd import ops
    n = 257
    _, W0 = _weights(n)
    off, hist, hw = EC.score_lists(n, N_LISTS, 10, 40, "positive")
    clean = ops.ease_scores(_cuda(W0), off, hist, hw)
    e = int(off[5]) + 1 if off[6] - off[5] > 1 else int(off[3]) + 1
    l_bad = int(np.searchsorted(off, e, "right") - 1)
    for what in ("item", "negative item", "offsets", "nan", "large term"):
        W, off2, hist2, hw2 = W0.copy(), off.copy(), hist.copy(), hw.copy()
        l = l_bad
        if what == "item":
            hist2[e] = n
        elif what == "negative item":
            hist2[e] = -1
        elif what == "offsets":
            l = 2
            off2[3] = off2[2] - 1                                       # list 2 is decreasing, list 3 starts earlier
        elif what == "nan":
            hw2[e] = np.nan
        else:
            W[hist2[e], 5] = 1025.0 / hw2[e]                            # that one term passes 1024
        want, err = R.ease_scores(W, off2, hist2, hw2)
        assert err == 1, what
        got, flag = ops.ease_scores(_cuda(W), off2, hist2, hw2, check=False)
        assert int(flag.item()) == 1, what
        assert np.array_equal(_u32(got), _u32(want)), what
        with pytest.raises(ValueError, match="out of range"):
            ops.ease_scores(_cuda(W), off2, hist2, hw2)
        others = [x for x in range(N_LISTS) if x != l and not (what == "offsets" and x == 3)]
        if what == "large term":
            others = [x for x in others if hist[e] not in hist[off[x]:off[x + 1]]]
            cols = np.arange(n) != 5
            assert np.array_equal(_u32(got)[l][cols], _u32(clean)[l][cols])    # the other terms of the entry count
        assert len(others) >= 6 and np.array_equal(_u32(got)[others], _u32(clean)[others]), what
        if what == "offsets":
            assert (_u32(got)[2] == NAN_BITS).all()


def test_inverse_weights_and_scores_replay_from_a_graph():
    """The three calls captured into one graph on one stream run nothing; the replay writes what the plain calls do"""
    import torch
    from anime_recommendations_amd import ops
    L = _lib()
    lib = L.load()
    n, n_l = _sizes("nb+1"), 5
    A = EC.gram_case(n, 50.0)
    off, hist, hw = EC.score_lists(n, n_l, 3, 30, "signed")
    P0, _ = ops.spd_inverse(_cuda(A))                                   # the kernels are loaded before the capture begins
    W0 = ops.ease_weights(P0)
    S0 = ops.ease_scores(W0, off, hist, hw)
    torch.cuda.synchronize()
    buf = _cuda(A)
    offd, histd, hwd = _cuda(off), _cuda(hist), _cuda(hw)
    shapes = ((n * n, torch.float32), (n_l * n, torch.float32), (1, torch.int32), (1, torch.int32))
    W, out, info, err = [poison.fill(torch.empty(m, dtype=dt, device="cuda"), 0x3F) for m, dt in shapes]
    ws = poison.fill(torch.empty(int(lib.anirec_spd_inverse_workspace_bytes(n)), dtype=torch.uint8, device="cuda"), 0x3F)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st = [lib.anirec_spd_inverse(L.ptr(buf), n, n, L.ptr(info), L.ptr(ws), ws.numel(), s),
              lib.anirec_ease_weights(L.ptr(buf), n, n, L.ptr(W), n, s),
              lib.anirec_ease_scores(L.ptr(W), n, n, L.ptr(offd), L.ptr(histd), L.ptr(hwd), n_l, len(hist), L.ptr(out), n,
                                     L.ptr(err), s)]
    assert st == [0, 0, 0]
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0x3F).all()) for t in (W, out, info, err))          # captured, not run
    assert np.array_equal(_u64(buf), _u64(A))
    graph.replay()
    torch.cuda.synchronize()
    assert int(info.item()) == 0 and int(err.item()) == 0
    assert np.array_equal(_u64(buf), _u64(P0)) and np.array_equal(_u32(W.view(n, n)), _u32(W0))
    assert np.array_equal(_u32(out.view(n_l, n)), _u32(S0))


# ---- the recs layer ---------------------------------------------------------------------------------------------------
def _planted_fit(reg=100.0, neighbours=0):
    from anime_recommendations_amd import recs
    c = EC.planted()
    return c, recs.ease_fit(c["user"], c["item"], np.ones(len(c["user"]), np.float32), c["n_users"], c["n_items"],
                            reg=reg, neighbours=neighbours)


def test_truncated_model_with_every_neighbour_is_the_dense_model():
    from anime_recommendations_amd import recs
    n, n_users = 65, 130
    _, B = EC.random_bits(n, n_users, 21)
    items, users = np.nonzero(B)
    fit = recs.ease_fit(users, items, np.ones(len(users), np.float32), n_users, n, reg=50.0, neighbours=n - 1)
    assert fit["knn"]["nbr_idx"].shape == (n, n - 1) and int(fit["knn"]["nbr_idx"].min()) >= 0
    off, hist, hw = EC.score_lists(n, 20, 4, 40, "signed")
    dense = recs.ease_rows_source(fit, off, hist, hw)(0, 20)
    knn = recs.itemknn_rows_source(fit["knn"], off, hist, hw)(0, 20)
    assert np.array_equal(_u32(dense), _u32(knn))
    want, err = R.ease_scores(fit["W"].cpu().numpy(), off, hist, hw)
    assert err == 0 and np.array_equal(_u32(dense), _u32(want))
    assert np.array_equal(fit["pop"].cpu().numpy(), B.sum(1))


def test_recs_routes_on_the_planted_blocks():
    import torch
    from anime_recommendations_amd import ops, recs
    c, fit = _planted_fit()
    n = c["n_items"]
    assert fit["n_liked"] == len(c["user"]) and fit["reg"] == 100.0 and fit["n_items"] == n and "knn" not in fit
    # the fit is the restatement's up to the inverse's rounding
    want_W = R.ease_weights(np.linalg.inv(R.gram_matrix(CR.pack_bits(c["B"]), c["n_users"], 100.0)))
    assert np.abs(_ordered(fit["W"].cpu().numpy()) - _ordered(want_W)).max() <= 1
    off, hist = EC.planted_histories(c)
    n_l = len(off) - 1
    seen = _cuda(CR.pack_bits(c["B"][:, c["held_user"]].T).view(np.int32))
    rows = ops.ease_scores(fit["W"], off, hist)
    for batch in (97, recs.EASE_BATCH):
        i1, s1 = recs.ease_topk(fit, off, hist, None, 10, seen, batch=batch)
        i2, s2 = ops.rows_topk(rows, 10, wbits=seen)
        assert torch.equal(i1, i2) and np.array_equal(_u32(s1), _u32(s2))
        r1 = recs.ease_rank(fit, off, hist, None, seen, np.arange(n_l), c["held_item"], batch=batch)
        assert torch.equal(r1, ops.rows_rank(rows, np.arange(n_l), c["held_item"], seen))
    rank = r1.cpu().numpy()
    want_rows, _ = R.ease_scores(fit["W"].cpu().numpy(), off, hist)
    assert np.array_equal(rank, R.ranks(want_rows, c["B"][:, c["held_user"]].T, np.arange(n_l), c["held_item"]))
    ease_hr, pop_hr = EC.hit_rate(rank), EC.popularity_hit_rate(c)
    print("hit rate @10: EASE %.4f, popularity %.4f" % (ease_hr, pop_hr))
    assert ease_hr > pop_hr
    q = np.asarray([0, 5, n - 1, 5])
    keep = np.ones(n, np.uint8)
    keep[::7] = 0
    for kp in (None, keep):
        i3, s3 = recs.ease_similar(fit, q, 8, keep=kp)
        i4, s4 = ops.rows_topk(fit["W"][_cuda(q)], 8, self_idx=q, keep=kp)
        assert torch.equal(i3, i4) and np.array_equal(_u32(s3), _u32(s4))
    assert not (i3.cpu().numpy() == q[:, None]).any()
    with pytest.raises(ValueError, match="out of range"):
        recs.ease_similar(fit, [n], 3)


def test_ease_fit_names_reg_when_the_matrix_is_not_positive_definite(monkeypatch):
    import torch
    from anime_recommendations_amd import ops, recs
    real = ops.spd_inverse
    monkeypatch.setattr(ops, "spd_inverse", lambda A, workspace=None: real(-A, workspace))
    with pytest.raises(ValueError, match="reg"):
        recs.ease_fit([0, 1], [0, 1], [1.0, 1.0], 2, 2, reg=1.0)
    torch.cuda.synchronize()


# ---- the components, on the recs fixture ------------------------------------------------------------------------------
def _fixture_frames(rec):
    from anime_recommendations_amd import components as C
    return C.load_anime_df(RF.csv(rec, "anime_csv")), C.load_synopses(RF.csv(rec, "synopses_csv"))


def test_evaluate_frame_baseline_ease_on_the_recs_fixture(fixture_store):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, data, recs, weights_io
    pq = fixture_store["pq"]
    ks = [1, 5, 20]
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    table = data.load_user_stats(pq)
    par = {"reg": 20.0, "min_rating": 0.5}
    frame, summary = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline=["ease", "popularity"], ease=par)
    assert frame.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity", "hit_rate_ease",
                                      "ndcg_ease"]
    assert {"ease_mrr", "ease_mean_rank", "ease_hit_rate@5", "ease_ndcg@20"} <= set(summary)
    pop_frame, pop = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline="popularity")
    assert frame[pop_frame.columns.tolist()].to_csv(index=False) == pop_frame.to_csv(index=False)
    assert {k: summary[k] for k in pop} == pop
    # the figures of the ease_rank route on the training slice
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    assert len(row) > 100
    tu, ta, tr = table.user[train], table.anime[train], table.rating[train]
    fit = recs.ease_fit(tu, ta, tr, table.n_users, table.n_anime, 0.5, 20.0)
    hoff, hist, _ = recs.history_csr(tu, ta, tr, users, 0.5)
    seen = recs.listed_seen_bits(tu, ta, users, table.n_users, table.n_anime)
    rank = recs.ease_rank(fit, hoff, hist, None, seen, row, anime).cpu().numpy()
    b = recs.ranking_metrics(rank, ks)
    assert frame["hit_rate_ease"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_ease"].tolist() == [b["ndcg"][k] for k in ks]
    assert summary["ease_mrr"] == b["mrr"] and summary["ease_mean_rank"] == b["mean_rank"]
    # and of the restatement's score rows of that fit
    want_rows, err = R.ease_scores(fit["W"].cpu().numpy(), hoff, hist)
    seen_b = CR.unpack_bits(seen.cpu().numpy().view(np.uint32), table.n_anime)
    assert err == 0 and np.array_equal(rank, R.ranks(want_rows, seen_b, row, anime))
    # the truncated model is another system: its ranks are the item-kNN route's over the fit's own tables
    knn_frame, _ = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline="ease", ease=dict(par, neighbours=5))
    fit5 = recs.ease_fit(tu, ta, tr, table.n_users, table.n_anime, 0.5, 20.0, 5)
    rank5 = recs.itemknn_rank(fit5["knn"], hoff, hist, None, seen, row, anime).cpu().numpy()
    b5 = recs.ranking_metrics(rank5, ks)
    assert knn_frame["hit_rate_ease"].tolist() == [b5["hit_rate"][k] for k in ks]
    # intervals
    ci_frame, ci = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline=["ease", "popularity"], ease=par,
                                    ci_replicates=100)
    assert {"hit_rate_diff_ease", "hit_rate_p_ease", "ndcg_ease_lo", "ndcg_ease_hi"} <= set(ci_frame.columns)
    assert {"ease_mrr_lo", "ease_mrr_hi", "mrr_diff_ease", "mrr_p_ease"} <= set(ci)
    assert ci_frame[frame.columns.tolist()].to_csv(index=False) == frame.to_csv(index=False)
    assert (ci_frame["ndcg_ease_lo"] <= ci_frame["ndcg_ease_hi"]).all()


def test_hybrid_recs_takes_ease_as_a_member(fixture_store):  # noqa: F811
    import torch
    from anime_recommendations_amd import artifacts, components as C, ops, recs, weights_io
    rec, df = fixture_store["rec"], fixture_store["df"]
    flags = rec["flags"]
    user = int(rec["model_recs"]["cases"][0]["user"])
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    anime_df, syn_df = _fixture_frames(rec)
    user_ids, anime_ids = C.index_tables(model, df)
    head = weights_io.model_head(model)
    types = C.literal(flags["MR_TYPES"])
    frame, stats = C.hybrid_recs_frame(model["U"], model["A"], head, user_ids, anime_ids, df, anime_df, syn_df, user, 15,
                                       types=types, systems=("model", "ease"), ease={"reg": 20.0})
    assert stats["hybrid_systems"] == ["model", "ease"] and len(frame) == 15
    assert frame.columns.tolist()[-3:] == ["Hybrid_score", "Rank_model", "Rank_ease"]
    # hybrid_topk on the two sources, under the list's own mask
    ui, ai, r = C.rating_indices(df, user_ids, anime_ids)
    urow = int(np.flatnonzero(np.asarray(user_ids) == user)[0])
    fit = recs.ease_fit(ui, ai, r, len(user_ids), len(anime_ids), 0.0, 20.0)
    hoff, hist, _ = recs.history_csr(ui, ai, r, [urow])
    meta = C.metadata_by_index(anime_ids, anime_df, syn_df)
    blocked = ~C.filter_mask(meta, anime_df, types) | ~C.unwatched_mask(df, anime_ids, user)
    bits = _cuda(CR.pack_bits(blocked[None]).view(np.int32))
    tU, tA = torch.as_tensor(model["U"]).cuda(), torch.as_tensor(model["A"]).cuda()
    sources = [recs.model_rows_source(tU, tA, head, [urow]), recs.ease_rows_source(fit, hoff, hist)]
    idx, fused = recs.hybrid_topk(sources, 15, watched_bits=bits)
    assert frame["anime_id"].tolist() == np.asarray(anime_ids)[idx.cpu().numpy()[0]].tolist()
    assert np.array_equal(_u32(frame["Hybrid_score"].to_numpy(np.float32)), _u32(fused.cpu().numpy()[0]))
    rank = ops.rows_rank(sources[1](0, 1), np.zeros(15, np.int64), idx[0], bits).cpu().numpy()
    assert frame["Rank_ease"].tolist() == (rank + 1).tolist()


def _er_argv(flags, **kw):
    al = dict(project_name="anime_recommendations", main_df="user_stats.parquet:latest", main_df_type="parquet",
              anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopses_df="synopses.csv:latest",
              sypnopsis_df_type="raw_data", anime_query="none", a_query_number=20, random_anime=False,
              anime_rec_genres=flags["SA_GENRES"], an_spec_genres=False, types=flags["SA_TYPES"], spec_types=False,
              a_rec_type="csv", save_sim_anime=True)
    argv = []
    for k, v in dict(al, **kw).items():
        argv += ["--" + k, str(v)]
    return argv


def test_ease_recs_component_in_both_modes(fixture_store, monkeypatch):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, recs
    work, rec, df = (fixture_store[k] for k in ("work", "rec", "df"))
    anime_df, syn_df = _fixture_frames(rec)
    monkeypatch.chdir(work)
    mod = load_component("ease_recs")
    parser = mod.make_parser()
    flags, query = rec["flags"], rec["similar_anime"]["cases"][0]["query"]
    types = C.literal(flags["SA_TYPES"])
    # an anime query: the largest weights of the query's row of W
    mod.go(parser.parse_args(_er_argv(flags, anime_query=query, spec_types=True, ease_reg=20, liked_min_rating=0.5)))
    fn = C.clean(query) + "_ease.csv"
    got = (work / fn).read_text()
    logged = artifacts.artifact_metadata(fn + ":latest")
    frame, frame_fn, stats = C.ease_similar_frame(df, anime_df, syn_df, query, 20, types=types, liked_min_rating=0.5,
                                                  reg=20.0)
    assert frame_fn == fn and got == frame.to_csv(index=False)
    assert logged["Queried anime"] == query and logged["reg"] == 20.0 and logged["n_items"] == stats["n_items"]
    liked = int((df.rating.to_numpy().astype(np.float32) >= np.float32(0.5)).sum())
    assert logged["liked_pairs"] == stats["liked_pairs"] == liked
    assert frame.columns.tolist() == ["Name", "Similarity", "Genres", "Sypnopsis", "Episodes", "Japanese name", "Studios",
                                      "Premiered", "Score", "Type", "Source", "Rating"]
    assert 0 < len(frame) <= 20 and query not in frame["Name"].tolist() and frame["Type"].isin(types).all()
    assert (np.diff(frame["Similarity"]) <= 0).all()
    user_ids, anime_ids = C.index_tables({}, df)
    ui, ai, r = C.rating_indices(df, user_ids, anime_ids)
    fit = recs.ease_fit(ui, ai, r, len(user_ids), len(anime_ids), 0.5, 20.0)
    meta = C.metadata_by_index(anime_ids, anime_df, syn_df)
    q = int(np.flatnonzero(np.asarray(anime_ids) == C.find_anime_id(query, anime_df))[0])
    wi, wv = CR.rows_topk(fit["W"][q:q + 1].cpu().numpy(), 20, self_idx=[q],
                          keep=C.filter_mask(meta, anime_df, types).astype(np.uint8))
    assert frame["Name"].tolist() == meta["Name"].to_numpy()[wi[0][wi[0] >= 0]].tolist()
    assert np.array_equal(_u32(frame["Similarity"].to_numpy(np.float32)), _u32(wv[0][wi[0] >= 0]))
    # a user query: that user's list among the anime they have not rated
    user = int(rec["model_recs"]["cases"][0]["user"])
    mod.go(parser.parse_args(_er_argv(flags, user_query=user, ease_reg=20)))
    got = (work / ("User_ID_%d_ease_recs.csv" % user)).read_text()
    frame, stats = C.ease_recs_frame(df, anime_df, syn_df, user, 20, reg=20.0)
    assert got == frame.to_csv(index=False) and len(frame) == 20 and "Ease_score" in frame.columns
    mine = df[df.user_id == user]
    assert not set(frame["anime_id"]) & set(mine.anime_id) and (np.diff(frame["Ease_score"]) <= 0).all()
    fit = recs.ease_fit(ui, ai, r, len(user_ids), len(anime_ids), 0.0, 20.0)
    pos = {a: i for i, a in enumerate(np.asarray(anime_ids).tolist())}
    urow = int(np.flatnonzero(np.asarray(user_ids) == user)[0])
    hoff, hist, _ = recs.history_csr(ui, ai, r, [urow])
    assert sorted(hist.tolist()) == sorted(pos[a] for a in mine.anime_id)
    scores, err = R.ease_scores(fit["W"].cpu().numpy(), hoff, hist)
    seen = np.zeros((1, len(anime_ids)), bool)
    seen[0, [pos[a] for a in mine.anime_id]] = True
    wi, wv = CR.rows_topk(scores, 20, keep=meta["has_meta"].to_numpy().astype(np.uint8), wbits=CR.pack_bits(seen))
    assert err == 0 and frame["anime_id"].tolist() == np.asarray(anime_ids)[wi[0]].tolist()
    assert np.array_equal(_u32(frame["Ease_score"].to_numpy(np.float32)), _u32(wv[0]))
    # the truncated model through the same component
    mod.go(parser.parse_args(_er_argv(flags, user_query=user, ease_reg=20, ease_neighbours=5)))
    knn_frame, knn_stats = C.ease_recs_frame(df, anime_df, syn_df, user, 20, reg=20.0, neighbours=5)
    assert (work / ("User_ID_%d_ease_recs.csv" % user)).read_text() == knn_frame.to_csv(index=False)
    assert knn_stats["neighbours"] == 5
    assert artifacts.artifact_metadata("User_ID_%d_ease_recs.csv:latest" % user)["neighbours"] == 5
    with pytest.raises(ValueError, match="exactly one"):
        mod.go(parser.parse_args(_er_argv(flags, user_query=user, anime_query="Naruto")))
