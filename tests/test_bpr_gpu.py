"""GPU tests of BPR matrix factorisation: anirec_bpr_sample and anirec_bpr_steps against the NumPy
restatement (tests/bpr_restatement.py) BIT FOR BIT at every width and at the batch, step, tries, bias and rate edges, the
error and argument rules, the whole fit, the lists and ranks, planted blocks, ``evaluate_frame(baseline="bpr")`` and the
hybrid member on the recs fixture."""
import functools

import numpy as np
import pytest
import torch

import bpr_restatement as R
import poison
import recs_fixture as RF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_USERS, N_ITEMS = 40, 97
RATES = ((0.05, 0.01), (0.5, 0.1))
# (batch, n_steps, tries, bias, rates): every batch, step count, tries, bias and rate pair of the issue at every width
CONFIGS = ((1, 20, 8, 1, 0), (63, 3, 1, 0, 1), (64, 1, 8, 0, 0), (65, 20, 1, 1, 1), (256, 3, 8, 1, 1), (1000, 20, 8, 0, 0),
           (1000, 1, 1, 1, 0), (256, 0, 8, 0, 1))


def _cuda(x, dtype=None):
    t = torch.as_tensor(np.array(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def lists():
    """(offsets, idx, pair_user): 40 users x 97 items; lists of 0, 1, 2, 33, 96 (all but one) and 97 (all) items, the rest
    random"""
    rng = np.random.default_rng(5)
    lens = [0, 1, 2, 33, 96, 97] + list(rng.integers(1, 40, N_USERS - 6))
    u = np.concatenate([np.full(n, r) for r, n in enumerate(lens)])
    i = np.concatenate([np.sort(rng.choice(N_ITEMS, n, replace=False)) for n in lens])
    off, idx, pu = R.csr(u, i, N_USERS, N_ITEMS)
    for a in (off, idx, pu):
        a.setflags(write=False)
    return off, idx, pu


@functools.lru_cache(maxsize=None)
def tables(width, scale=0.3):
    rng = np.random.default_rng(width)
    X = (rng.standard_normal((N_USERS, width)) * scale).astype(np.float32)
    Y = (rng.standard_normal((N_ITEMS, width)) * scale).astype(np.float32)
    X[:, -1] = 1.0
    X.setflags(write=False), Y.setflags(write=False)
    return X, Y


def _steps(X, Y, csr, batch, tries, seed, step0, n_steps, lr, reg, bias, **kw):
    """(X', Y', counts, flag) of ops.bpr_steps on copies of the tables"""
    from anime_recommendations_amd import ops
    Xd, Yd = _cuda(X), _cuda(Y)
    counts, err = ops.bpr_steps(Xd, Yd, *csr, batch, tries, seed, step0, n_steps, lr, reg, bias, check=False, **kw)
    return Xd.cpu().numpy(), Yd.cpu().numpy(), counts.cpu().numpy(), int(err.item())


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the sampler ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,tries,seed,step0,n_steps", [(1, 1, 0, 0, 1), (63, 8, 1, 0, 3), (64, 16, 2, 5, 2),
                                                            (65, 8, 2 ** 32 - 1, 2 ** 31 - 3, 2), (1000, 8, 7, 100, 4),
                                                            (256, 1, 7, 0, 0)])
def test_sample_equals_the_restatement(batch, tries, seed, step0, n_steps):
    from anime_recommendations_amd import ops
    off, idx, pu = lists()
    got = ops.bpr_sample(off, idx, pu, N_ITEMS, batch, tries, seed, step0, n_steps).cpu().numpy()
    want = R.sample(off, idx, pu, N_ITEMS, batch, tries, seed, step0, n_steps)
    assert _same(got, want)
    if n_steps:
        u, j = got[..., 0], got[..., 2]
        assert (j[u == 5] == -1).all()                           # the user who likes everything drops every slot
        assert (np.diff(off)[u[j >= 0]] < N_ITEMS).all()


# ---- steps, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", R.WIDTHS)
def test_steps_equal_the_restatement_bit_for_bit(width):
    csr = lists()
    X, Y = tables(width)
    for batch, n_steps, tries, bias, rate in CONFIGS:
        lr, reg = RATES[rate]
        gx, gy, gc, ge = _steps(X, Y, csr, batch, tries, 3, 2, n_steps, lr, reg, bias)
        wx, wy, wc, we = R.steps(X, Y, *csr, batch, tries, 3, 2, n_steps, lr, reg, bias)
        what = (width, batch, n_steps, tries, bias, lr, reg)
        assert ge == we, what
        assert _same(gc, wc), (what, gc, wc)
        assert _same(gx, wx) and _same(gy, wy), (what, int((gx != wx).sum()), int((gy != wy).sum()))
        if bias:
            assert (gx[:, -1] == 1.0).all()
        if n_steps == 0:
            assert _same(gx, X) and _same(gy, Y)                 # no step: the tables untouched


def test_one_row_touched_by_every_slot_of_a_batch():
    """every positive on a single item: item 5's row collects a term from every kept slot of the step"""
    off, idx, pu = R.csr(np.arange(N_USERS), np.full(N_USERS, 5), N_USERS, N_ITEMS)
    X, Y = tables(64)
    gx, gy, gc, ge = _steps(X, Y, (off, idx, pu), 256, 8, 1, 0, 3, 0.05, 0.01, 1)
    wx, wy, wc, we = R.steps(X, Y, off, idx, pu, 256, 8, 1, 0, 3, 0.05, 0.01, 1)
    assert ge == we == 0 and _same(gc, wc) and wc[0, 0] > 250
    assert _same(gx, wx) and _same(gy, wy)


def test_split_chain_repeat_and_stale_workspace_give_the_same_bits():
    from anime_recommendations_amd import ops
    csr = lists()
    X, Y = tables(128)
    one = _steps(X, Y, csr, 65, 8, 9, 4, 7, 0.05, 0.01, 1)
    assert all(_same(a, b) for a, b in zip(one[:3], _steps(X, Y, csr, 65, 8, 9, 4, 7, 0.05, 0.01, 1)[:3]))     # run to run
    ax, ay, ac, _ = _steps(X, Y, csr, 65, 8, 9, 4, 3, 0.05, 0.01, 1)                     # steps 4 .. 6, then 7 .. 10
    bx, by, bc, _ = _steps(ax, ay, csr, 65, 8, 9, 7, 4, 0.05, 0.01, 1)
    assert _same(bx, one[0]) and _same(by, one[1]) and _same(np.concatenate([ac, bc]), one[2])
    for byte in poison.ORDER:
        with poison.poisoned(byte, []):
            dirty = _steps(X, Y, csr, 65, 8, 9, 4, 7, 0.05, 0.01, 1)
        assert all(_same(a, b) for a, b in zip(one[:3], dirty[:3])) and dirty[3] == 0, hex(byte)
        ws = poison.fill(torch.empty(ops.bpr_workspace_bytes(N_USERS, N_ITEMS, 128, 65) + 64, dtype=torch.uint8,
                                     device=DEV), byte)
        given = _steps(X, Y, csr, 65, 8, 9, 4, 7, 0.05, 0.01, 1, workspace=ws)
        assert all(_same(a, b) for a, b in zip(one[:3], given[:3])), hex(byte)


def test_bpr_fit_equals_the_restatements_fit_bit_for_bit():
    from anime_recommendations_amd import recs
    rng = np.random.default_rng(2)
    like = rng.random((30, 23)) < 0.3
    u, i = np.nonzero(like)
    u, i = np.concatenate([u, u[:9]]), np.concatenate([i, i[:9]])     # repeats count once
    par = dict(factors=32, epochs=2, batch=64, lr=0.05, reg=0.01, tries=8, bias=True, seed=4)
    fit = recs.bpr_fit(u, i, 30, 23, **par)
    X, Y, counts = R.fit(u, i, 30, 23, **par)
    assert _same(fit["X"].cpu().numpy(), X) and _same(fit["Y"].cpu().numpy(), Y)
    assert fit["counts"] == counts.tolist() and fit["n_pairs"] == int(like.sum())
    assert {k: fit[k] for k in par} == par
    again = recs.bpr_fit(u, i, 30, 23, **par)
    assert torch.equal(again["X"], fit["X"]) and torch.equal(again["Y"], fit["Y"])


# ---- error rules ------------------------------------------------------------------------------------------------------
def test_an_index_out_of_range_flags_and_is_not_followed():
    from anime_recommendations_amd import ops
    off, idx, pu = lists()
    X, Y = tables(32)
    clean = ops.bpr_sample(off, idx, pu, N_ITEMS, 1000, 8, 1, 0, 1).cpu().numpy()[0]
    h = R.slot_hash(1, 0, np.arange(1000))
    p = R.pick(R.draw(h, 0), len(idx))
    for where, bad in (("idx", N_ITEMS), ("idx", -1), ("pair_user", N_USERS), ("pair_user", -7), ("idx", 2 ** 31 - 1)):
        entry = int(p[17])
        b_idx, b_pu = idx.copy(), pu.copy()
        (b_idx if where == "idx" else b_pu)[entry] = bad
        trip, err = ops.bpr_sample(off, b_idx, b_pu, N_ITEMS, 1000, 8, 1, 0, 1, check=False)
        trip = trip.cpu().numpy()[0]
        hit = p == entry
        assert int(err.item()) == ops._lib.BPR_ERR_INDEX and (trip[hit] == -1).all()
        other = ~hit & (clean[:, 0] != pu[entry])                # the slots of other users draw what they drew
        assert _same(trip[other], clean[other])
        with pytest.raises(ValueError, match="out of range"):
            ops.bpr_sample(off, b_idx, b_pu, N_ITEMS, 1000, 8, 1, 0, 1)
        gx, gy, gc, ge = _steps(X, Y, (off, b_idx, b_pu), 1000, 8, 1, 0, 1, 0.05, 0.01, 0)
        assert ge & ops._lib.BPR_ERR_INDEX and np.isfinite(gx).all() and np.isfinite(gy).all()
        assert gc[0, 0] + gc[0, 1] == 1000 and gc[0, 1] >= hit.sum()
        with pytest.raises(ValueError, match="out of range"):
            ops.bpr_steps(_cuda(X), _cuda(Y), off, b_idx, b_pu, 1000, 8, 1, 0, 1, 0.05, 0.01, 0)


def test_a_term_above_2_pow_20_sets_the_divergence_bit():
    from anime_recommendations_amd import ops
    csr = lists()
    X, Y = tables(32)
    bigY = (Y * np.float32(3e7)).astype(np.float32)              # d = y_i - y_j ~ 1e7: g d breaks the guard where g is not 0
    bigX = -np.abs(X)                                            # keeps some x^ negative or small: g near 1 somewhere
    gx, gy, gc, ge = _steps(bigX, bigY, csr, 256, 8, 0, 0, 1, 0.05, 0.01, 0)
    wx, wy, wc, we = R.steps(bigX, bigY, *csr, 256, 8, 0, 0, 1, 0.05, 0.01, 0)
    assert we == R.ERR_DIVERGED and ge == we and _same(gc, wc) and _same(gx, wx) and _same(gy, wy)
    with pytest.raises(ValueError, match="diverged"):
        ops.bpr_steps(_cuda(bigX), _cuda(bigY), *csr, 256, 8, 0, 0, 1, 0.05, 0.01, 0)


def test_einval_and_eworkspace_write_nothing():
    from anime_recommendations_amd import ops
    lib, ptr = ops._lib.load(), ops._lib.ptr
    off, idx, pu = (_cuda(a) for a in lists())
    X0, Y0 = tables(64)
    nnz, need = len(lists()[1]), ops.bpr_workspace_bytes(N_USERS, N_ITEMS, 64, 100)
    good = dict(n_users=N_USERS, n_items=N_ITEMS, width=64, nnz=nnz, batch=100, tries=8, step0=0, n_steps=2, lr=0.05,
                reg=0.01, bias=1, ws_bytes=need)
    bad = [dict(width=48), dict(n_users=0), dict(n_items=0), dict(nnz=0), dict(nnz=2 ** 31), dict(batch=0), dict(tries=0),
           dict(tries=17), dict(step0=-1), dict(n_steps=-1), dict(step0=2 ** 31 - 2, n_steps=2), dict(lr=-1.0),
           dict(lr=float("nan")), dict(reg=float("inf")), dict(bias=2), dict(null="X"), dict(null="Y"),
           dict(null="offsets"), dict(null="idx"), dict(null="pu"), dict(null="err"), dict(null="ws"), dict(null="counts"),
           dict(shift="X"), dict(shift="Y"), dict(shift="ws"), dict(shift="counts"),     # 4 bytes off: not 16- / 8-aligned
           dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    for change in bad:
        a = dict(good, **{k: v for k, v in change.items() if k not in ("null", "shift")})
        X, Y = _cuda(X0), _cuda(Y0)
        counts = poison.fill(torch.empty(2, 3, dtype=torch.int64, device=DEV), 0x3F)
        err = poison.fill(torch.empty(1, dtype=torch.int32, device=DEV), 0x3F)
        ws = poison.fill(torch.empty(need + 8, dtype=torch.uint8, device=DEV), 0x3F)
        named = dict(X=X, Y=Y, offsets=off, idx=idx, pu=pu, counts=counts, err=err, ws=ws)

        def arg(name):      # the pointer as passed: NULL, 4 bytes past the tensor's start, or the tensor's
            if change.get("null") == name:
                return None
            return ptr(named[name]) + (4 if change.get("shift") == name else 0)
        status = lib.anirec_bpr_steps(arg("X"), arg("Y"), a["n_users"], a["n_items"], a["width"], arg("offsets"),
                                      arg("idx"), arg("pu"), a["nnz"], a["batch"], a["tries"], 0, a["step0"], a["n_steps"],
                                      a["lr"], a["reg"], a["bias"], arg("counts"), arg("err"), arg("ws"), a["ws_bytes"],
                                      ops._stream())
        want = "workspace" if "ws_bytes" in change else "invalid"
        assert status != 0 and want in lib.anirec_status_string(status).decode().lower(), change
        torch.cuda.synchronize()
        assert _same(X.cpu().numpy(), X0) and _same(Y.cpu().numpy(), Y0), change
        for t in (counts, err, ws):
            assert bool((t.view(torch.uint8) == 0x3F).all()), change
    assert lib.anirec_bpr_workspace_bytes(N_USERS, N_ITEMS, 48, 100) == 0
    assert lib.anirec_bpr_workspace_bytes(N_USERS, N_ITEMS, 64, 0) == 0
    with pytest.raises(ValueError, match="offsets"):
        ops.bpr_steps(_cuda(X0), _cuda(Y0), [0, 3, 2] + [2] * (N_USERS - 2), lists()[1][:2], lists()[2][:2], 10)


# ---- lists and ranks --------------------------------------------------------------------------------------------------
def test_bpr_topk_and_bpr_rank_are_rows_topk_and_rows_rank_on_dot_scores():
    from anime_recommendations_amd import ops, recs
    rng = np.random.default_rng(9)
    n_users, n_items, dim = 150, 333, 64
    fit = {"X": _cuda(rng.standard_normal((n_users, dim)).astype(np.float32)),
           "Y": _cuda(rng.standard_normal((n_items, dim)).astype(np.float32))}
    users = rng.permutation(n_users)[:70]
    seen = _cuda(rng.integers(0, 2 ** 31, (70, (n_items + 31) // 32)).astype(np.int32) &
                 rng.integers(0, 2 ** 31, (70, (n_items + 31) // 32)).astype(np.int32))
    rows = ops.dot_scores(fit["X"][_cuda(users)], fit["Y"])
    tr, ta = rng.integers(0, 70, 400), rng.integers(0, n_items, 400)
    for watched in (None, seen):
        want_i, want_s = ops.rows_topk(rows, 12, wbits=watched)
        for batch in (recs.BPR_BATCH, 23):
            got_i, got_s = recs.bpr_topk(fit, users, 12, watched, batch=batch)
            assert torch.equal(got_i, want_i) and got_s.cpu().numpy().tobytes() == want_s.cpu().numpy().tobytes()
            assert torch.equal(recs.bpr_rank(fit, users, watched, tr, ta, batch=batch), ops.rows_rank(rows, tr, ta, watched))
    assert torch.equal(recs.bpr_rows_source(fit, users)(3, 9), rows[3:9])


# ---- planted blocks ---------------------------------------------------------------------------------------------------
def test_planted_blocks_bpr_ranks_the_held_out_pairs_above_popularity():
    """tests/test_bpr_cpu.py shows the gap on the restatement first: mean ranks 5.1 .. 5.7 (BPR), 14.4 .. 17.0 (popularity)"""
    from anime_recommendations_amd import ops, recs
    tu, ti, hu, hi = R.block_pairs(0)
    fit = recs.bpr_fit(tu, ti, **R.BLOCK)
    seen = recs.listed_seen_bits(tu, ti, hu, R.BLOCK["n_users"], R.BLOCK["n_items"])
    bpr_rank = recs.bpr_rank(fit, hu, seen, np.arange(len(hu)), hi).cpu().numpy()
    pop = recs.popularity_scores(ti, R.BLOCK["n_items"], R.BLOCK["n_users"]).to(DEV)
    pop_rank = ops.score_rank(pop, len(hu), np.arange(len(hu)), hi, watched_bits=seen).cpu().numpy()
    print("planted blocks: mean rank BPR %.2f, popularity %.2f" % (bpr_rank.mean(), pop_rank.mean()))
    assert bpr_rank.mean() < pop_rank.mean()


# ---- evaluate and the hybrid ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recs_table(tmp_path_factory):
    from anime_recommendations_amd import components as C, data, weights_io
    work = tmp_path_factory.mktemp("bpr")
    rec = RF.load()
    z, df = rec["npz"], RF.ratings(rec)
    user_ids, anime_ids = C.index_tables({}, df)
    pq, mp = str(work / "user_stats.parquet"), str(work / "wandb_anime_nn.h5")
    df.to_parquet(pq, index=False)
    weights_io.save_model(mp, z["U"], z["A"], dict(rec["model_recs"]["heads"]["sigmoid"], activation="sigmoid"),
                          user_ids=user_ids, anime_ids=anime_ids)
    return weights_io.load_model(mp), data.load_user_stats(pq), rec, df


def test_evaluate_frame_baseline_bpr_on_the_recs_fixture(recs_table):
    from anime_recommendations_amd import components as C, recs
    model, table, _, _ = recs_table
    ks = [1, 5, 20]
    par = dict(factors=32, epochs=2, batch=512, lr=0.05, reg=0.02, tries=4, bias=True, min_rating=0.6, seed=3)
    als_frame, als = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline=["als", "popularity"],
                                      als=dict(factors=32, sweeps=1))
    frame, summary = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline=["bpr", "popularity"], bpr=par)
    assert frame.columns.tolist() == [c.replace("_als", "_bpr") for c in als_frame.columns]
    assert list(summary) == [k.replace("als_", "bpr_") for k in als]
    # the bpr columns are a direct fit and rank with the same parameters
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    assert len(row) > 100
    tu, ta, tr = (np.asarray(c[train]) for c in (table.user, table.anime, table.rating))
    liked = tr.astype(np.float32) >= np.float32(0.6)
    fit = recs.bpr_fit(tu[liked], ta[liked], table.n_users, table.n_anime, 32, 2, 512, 0.05, 0.02, 4, True, seed=3)
    seen = recs.listed_seen_bits(tu, ta, users, table.n_users, table.n_anime)
    b = recs.ranking_metrics(recs.bpr_rank(fit, users, seen, row, anime), ks)
    assert frame["hit_rate_bpr"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_bpr"].tolist() == [b["ndcg"][k] for k in ks]
    assert summary["bpr_mrr"] == b["mrr"] and summary["bpr_mean_rank"] == b["mean_rank"]
    ci_frame, ci = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline="bpr", bpr=par, ci_replicates=50, ci_seed=1)
    for col in ("hit_rate_bpr_lo", "hit_rate_bpr_hi", "ndcg_bpr_lo", "ndcg_bpr_hi", "hit_rate_diff_bpr",
                "hit_rate_diff_bpr_lo", "hit_rate_diff_bpr_hi", "hit_rate_p_bpr", "ndcg_diff_bpr", "ndcg_p_bpr"):
        assert col in ci_frame.columns, col
    for key in ("bpr_mrr_lo", "bpr_mrr_hi", "bpr_mean_rank_lo", "bpr_mean_rank_hi", "mrr_diff_bpr", "mrr_p_bpr"):
        assert key in ci, key
    assert ci_frame["hit_rate_bpr"].tolist() == frame["hit_rate_bpr"].tolist()
    assert ci["bpr_mrr_lo"] <= ci["bpr_mrr"] <= ci["bpr_mrr_hi"] and 0.0 <= ci["mrr_p_bpr"] <= 1.0


def test_hybrid_recs_frame_takes_bpr_as_a_member(recs_table):
    from anime_recommendations_amd import components as C, recs, weights_io
    model, _, rec, df = recs_table
    anime_df, syn_df = C.load_anime_df(RF.csv(rec, "anime_csv")), C.load_synopses(RF.csv(rec, "synopses_csv"))
    user = int(rec["model_recs"]["cases"][0]["user"])
    user_ids, anime_ids = C.index_tables(model, df)
    head = weights_io.model_head(model)
    par = dict(factors=32, epochs=2, batch=512, seed=1)
    frame, stats = C.hybrid_recs_frame(model["U"], model["A"], head, user_ids, anime_ids, df, anime_df, syn_df, user, 15,
                                       systems=("model", "bpr"), bpr=par)
    assert stats["hybrid_systems"] == ["model", "bpr"] and len(frame) == 15
    assert frame.columns.tolist()[-3:] == ["Hybrid_score", "Rank_model", "Rank_bpr"]
    assert (np.diff(frame["Hybrid_score"]) <= 0).all() and (frame[["Rank_model", "Rank_bpr"]] >= 1).all().all()
    # the fused ranks of the listed anime are recs.hybrid_rank's over the same two sources under the same mask
    row, _, bits, tU, tA, _ = C._candidates(model["U"], model["A"], user_ids, anime_ids, df, anime_df, syn_df, user, 15,
                                            None, None)
    ui, ai, _ = C.rating_indices(df, user_ids, anime_ids)
    fit = recs.bpr_fit(ui, ai, len(user_ids), len(anime_ids),          # min_rating 0: every rating is a liked pair
                       **{k: v for k, v in dict(C.BPR_DEFAULTS, **par).items() if k != "min_rating"})
    sources = [recs.model_rows_source(tU, tA, head, [row]), recs.bpr_rows_source(fit, [row])]
    listed = pd_index(anime_ids, frame["anime_id"])
    wbits = torch.as_tensor(bits, device=DEV).reshape(1, -1)
    rank = recs.hybrid_rank(sources, wbits, np.zeros(15, np.int64), listed).cpu().numpy()
    assert rank.tolist() == list(range(15))


def pd_index(anime_ids, ids):
    import pandas as pd
    return pd.Index(np.asarray(anime_ids)).get_indexer(np.asarray(ids)).astype(np.int64)
