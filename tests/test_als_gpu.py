"""GPU tests of implicit-feedback ALS: anirec_als_gram against its derived bound, anirec_als_half_sweep
against the fp64 restatement within 8 x the fp32 restatement's recorded distance on the same case (tests/als_cases.py),
the exactness and error rules bit for bit, anirec_dot_scores against the fma chain, the whole fit, the lists and ranks,
planted blocks, and ``evaluate_frame(baseline="als")`` on the recs fixture."""
import numpy as np
import pytest
import torch

import als_cases as K
import als_restatement as R
import poison
import recs_fixture as RF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _cuda(x, dtype=None):
    t = torch.as_tensor(np.array(x))                            # a copy: the cases' arrays are read-only
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _sweep(case, check=True, **over):
    """ops.als_half_sweep on a case's inputs (the restatement's own G); ``over`` replaces inputs by name"""
    from anime_recommendations_amd import ops
    Y, G, off, idx, ex, alpha, start, lam, steps = K.case_inputs(case)
    a = dict(Y=Y, G=G, off=off, idx=idx, ex=ex, start=start)
    a.update(over)
    return ops.als_half_sweep(_cuda(a["Y"]), _cuda(a["G"]), np.array(a["off"]), np.array(a["idx"]), _cuda(a["start"]), lam,
                              steps, excess=None if a["ex"] is None else _cuda(a["ex"]), alpha=alpha, check=check)


# ---- Gram ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", K.WIDTHS)
@pytest.mark.parametrize("n", (1, 97, 1024, 1025, 2500))        # one row; the cases' table; a chunk, one past it, three chunks
def test_gram_is_within_its_derived_bound_and_reproducible(dim, n):
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(dim + n)
    Y = K.table(dim) if n == 97 else (rng.standard_normal((n, dim)) * rng.choice([0.01, 1.0, 30.0], (n, 1))).astype(np.float32)
    Yd = _cuda(Y)
    G = ops.als_gram(Yd)
    g, g64 = G.cpu().numpy().astype(np.float64), R.gram64(Y)
    slack = np.abs(g - g64) - R.gram_bound(Y)
    print("gram dim %d n %d: largest |g - g64| / bound %.3f" % (dim, n, (np.abs(g - g64) / R.gram_bound(Y)).max()))
    assert (slack <= 0).all(), slack.max()
    assert (g == g.T).all()                                      # a cell and its mirror add the same products in the same order
    assert torch.equal(ops.als_gram(Yd), G)
    for byte in poison.ORDER:
        with poison.poisoned(byte, []):
            again = ops.als_gram(Yd)
        assert torch.equal(again, G), hex(byte)


# ---- half-sweep parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: "w%d-p%d-s%d-%s" % (c[0], c[1], c[2], "per" if c[3] else "alpha"))
def test_half_sweep_is_within_8x_the_fp32_restatements_distance(case):
    X64, l64 = K.reference(case, "float64")
    rows, loss = _sweep(case)
    rows, loss = rows.cpu().numpy(), loss.cpu().numpy()
    row_tol, loss_tol = K.tolerances(case)
    dr, dl = float(np.abs(rows - X64).max()), float(np.abs(loss - l64).max())
    X32, l32 = K.reference(case, "float32")
    print("case %r: kernel-fp64 row %.3e (tol %.3e) loss %.3e (tol %.3e); kernel == fp32 restatement on %d / %d rows"
          % (case, dr, row_tol, dl, loss_tol, int((rows == X32).all(1).sum()), len(rows)))
    assert dr <= row_tol and dl <= loss_tol
    if case[2] == 0:                                             # no step: the start rows bit for bit, the loss at them
        empty = np.diff(K.rows(case[0])[0]) == 0
        assert rows[~empty].tobytes() == K.rows(case[0])[3][~empty].tobytes()


# ---- exactness and error rules -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", K.WIDTHS)
def test_empty_list_gives_zero_and_a_row_does_not_depend_on_its_company(dim):
    from anime_recommendations_amd import ops
    case = (dim, 1, 3, True)
    Y, G, off, idx, ex, alpha, start, lam, steps = K.case_inputs(case)
    rows, loss = _sweep(case)
    lens = np.diff(off)
    for u in np.flatnonzero(lens == 0):
        assert not rows[u].cpu().numpy().any() and not np.signbit(rows[u].cpu().numpy()).any() and float(loss[u]) == 0.0
    assert torch.equal(_sweep(case)[0], rows) and torch.equal(_sweep(case)[1], loss)       # run to run
    # reversed: the rows in the opposite order (ops then hands them out in another order as well)
    rev = np.arange(len(lens))[::-1]
    r_off = np.concatenate([[0], np.cumsum(lens[rev])])
    r_idx = np.concatenate([idx[off[u]:off[u + 1]] for u in rev])
    r_ex = np.concatenate([ex[off[u]:off[u + 1]] for u in rev])
    r_rows, r_loss = _sweep(case, off=r_off, idx=r_idx, ex=r_ex, start=start[rev])
    assert torch.equal(r_rows.flip(0), rows) and torch.equal(r_loss.flip(0), loss)
    # alone: each of a few rows in a call of its own, the long one among them
    for u in (1, 5, 9, K.LONG_ROW, len(lens) - 1):
        one_rows, one_loss = _sweep(case, off=np.array([0, lens[u]]), idx=idx[off[u]:off[u + 1]], ex=ex[off[u]:off[u + 1]],
                                    start=start[u:u + 1])
        assert torch.equal(one_rows[0], rows[u]) and torch.equal(one_loss[0], loss[u]), u
    # any order of the workgroups, and none: the C call itself
    lib, ptr = ops._lib.load(), ops._lib.ptr
    Yd, Gd, offd, idxd, exd = _cuda(Y), _cuda(G), _cuda(off), _cuda(idx), _cuda(ex)
    rng = np.random.default_rng(dim)
    for order in (None, np.arange(len(lens)), rng.permutation(len(lens)), rng.permutation(len(lens))):
        od = None if order is None else _cuda(order, torch.int32)
        for byte in (0x00, 0xFF):                                # the outputs and the flag word hold anything on entry
            x = _cuda(start).clone()
            ls = poison.fill(torch.empty(len(lens), dtype=torch.float32, device=DEV), byte)
            err = poison.fill(torch.empty(1, dtype=torch.int32, device=DEV), byte)
            ops._lib.check(lib.anirec_als_half_sweep(ptr(Yd), len(Y), dim, ptr(Gd), ptr(offd), ptr(idxd), ptr(exd), alpha,
                                                     ptr(od), ptr(x), len(lens), lam, steps, ptr(ls), ptr(err),
                                                     ops._stream()), "anirec_als_half_sweep")
            assert int(err.item()) == 0 and torch.equal(x, rows) and torch.equal(ls, loss)
    # an order entry out of range flags and is not followed
    od = _cuda(np.array([0, len(lens)] + list(range(2, len(lens))), np.int32))
    x, err = _cuda(start).clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
    ls = torch.zeros(len(lens), dtype=torch.float32, device=DEV)
    ops._lib.check(lib.anirec_als_half_sweep(ptr(Yd), len(Y), dim, ptr(Gd), ptr(offd), ptr(idxd), ptr(exd), alpha, ptr(od),
                                             ptr(x), len(lens), lam, steps, ptr(ls), ptr(err), ops._stream()), "order")
    assert int(err.item()) == 1 and torch.equal(x[2:], rows[2:]) and torch.equal(x[0], rows[0])
    assert torch.equal(x[1], _cuda(start)[1])                    # the row no workgroup took is untouched


@pytest.mark.parametrize("dim", (32, 256))
def test_bad_index_flags_and_poisons_its_row_alone(dim):
    case = (dim, 0, 2, False)
    off, idx = K.rows(dim)[0], K.rows(dim)[1]
    good_rows, good_loss = _sweep(case)
    last = int(np.flatnonzero(np.diff(off) > 0)[-1])             # the last row that has entries
    for u, bad in ((5, K.N_ITEMS), (K.LONG_ROW, -1), (last, 2 ** 31 - 1)):
        broken = idx.copy()
        broken[off[u] + (off[u + 1] - off[u]) // 2] = bad
        rows, loss, err = _sweep(case, check=False, idx=broken)
        assert int(err.item()) == 1
        assert torch.isnan(rows[u]).all() and torch.isnan(loss[u])
        keep = torch.arange(len(off) - 1, device=DEV) != u
        assert torch.equal(rows[keep], good_rows[keep]) and torch.equal(loss[keep], good_loss[keep])
        with pytest.raises(ValueError, match="out of range"):
            _sweep(case, idx=broken)
    from anime_recommendations_amd import ops
    Y, G, _, _, _, alpha, start, lam, steps = K.case_inputs(case)
    # a decreasing offsets pair, which the wrapper refuses, through the C call itself: row 3 ends before it starts (its row
    # and loss NaN, nothing read through the pair), row 4 then starts one entry early (inside the entries: another list,
    # another row), every other row as in a clean call
    lib, ptr = ops._lib.load(), ops._lib.ptr
    off2 = off.copy()
    off2[4] = off2[3] - 1
    x, err = _cuda(start).clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
    ls = torch.zeros(len(off) - 1, dtype=torch.float32, device=DEV)
    Yd, Gd, offd, idxd = _cuda(Y), _cuda(G), _cuda(off2), _cuda(idx)
    ops._lib.check(lib.anirec_als_half_sweep(ptr(Yd), len(Y), dim, ptr(Gd), ptr(offd), ptr(idxd), None, alpha, None, ptr(x),
                                             len(off) - 1, lam, steps, ptr(ls), ptr(err), ops._stream()), "bad pair")
    keep = torch.tensor([u not in (3, 4) for u in range(len(off) - 1)], device=DEV)
    assert int(err.item()) == 1 and torch.isnan(x[3]).all() and torch.isnan(ls[3])
    assert torch.equal(x[keep], good_rows[keep]) and torch.equal(ls[keep], good_loss[keep]) and not torch.isnan(x[4]).any()
    with pytest.raises(ValueError, match="offsets"):
        ops.als_half_sweep(_cuda(Y), _cuda(G), [0, 3, 2] + [2] * (len(off) - 3), np.array(idx[:2]), _cuda(start), lam, steps)
    with pytest.raises(ValueError, match="excess"):
        ops.als_half_sweep(_cuda(Y), _cuda(G), np.array(off), np.array(idx), _cuda(start), lam, steps,
                           excess=np.where(np.arange(len(idx)) == 7, -1.0, 1.0))


@pytest.mark.parametrize("byte", poison.ORDER)
def test_half_sweep_ignores_what_its_buffers_held(byte):
    case = (64, 1, 2, True)
    rows, loss = _sweep(case)
    with poison.poisoned(byte, []):
        d_rows, d_loss = _sweep(case)
    assert torch.equal(d_rows, rows) and torch.equal(d_loss, loss)


# ---- scores -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", K.WIDTHS)
@pytest.mark.parametrize("n_q,n,ld", [(1, 97, 97), (16, 130, 130), (17, 63, 70), (70, 129, 129), (130, 65, 200)])
def test_dot_scores_is_the_fma_chain_bit_for_bit(dim, n_q, n, ld):
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(dim * 1000 + n_q)
    Q = (rng.standard_normal((n_q, dim)) * 0.7).astype(np.float32)       # rows that are not normalised
    Y = (rng.standard_normal((n, dim)) * 1.3).astype(np.float32)
    out = poison.fill(torch.empty(n_q, ld, dtype=torch.float32, device=DEV), 0x7F)
    back = ops.dot_scores(_cuda(Q), _cuda(Y), out=out)
    assert back is out
    got = out.cpu().numpy()
    assert got[:, :n].tobytes() == R.dot_chain(Q, Y).tobytes()
    assert (got[:, n:].view(np.uint32) == 0x7F7F7F7F).all()             # nothing is written past column n
    if ld == n:
        assert torch.equal(ops.dot_scores(_cuda(Q), _cuda(Y)), out)


# ---- the whole fit --------------------------------------------------------------------------------------------------------
def test_als_fit_follows_the_fp32_restatement_and_its_loss_never_rises():
    from anime_recommendations_amd import recs
    u, i = K.fit_pairs()
    fit = recs.als_fit(u, i, **K.FIT)
    X32, Y32, l32 = K.fit_reference("float32")
    _, _, l64 = K.fit_reference("float64")
    dx = float(np.abs(fit["X"].cpu().numpy() - X32).max())
    dy = float(np.abs(fit["Y"].cpu().numpy() - Y32).max())
    dl = max(abs(a - b) / abs(b) for a, b in zip(fit["loss"], l32))
    print("als_fit against the fp32 restatement: X %.3e Y %.3e loss (relative) %.3e; tolerances %s"
          % (dx, dy, dl, tuple(8 * v for v in K.FIT_DEV)))
    assert dx <= 8 * K.FIT_DEV[0] and dy <= 8 * K.FIT_DEV[1] and dl <= 8 * K.FIT_DEV[2]
    assert len(fit["loss"]) == 2 * K.FIT["sweeps"]
    for t in range(1, len(l64)):
        if l64[t - 1] - l64[t] > K.FIT_MIN_DECREASE * l64[t - 1]:
            assert fit["loss"][t] <= fit["loss"][t - 1], (t, fit["loss"])
    again = recs.als_fit(u, i, **K.FIT)
    assert torch.equal(again["X"], fit["X"]) and torch.equal(again["Y"], fit["Y"]) and again["loss"] == fit["loss"]
    assert {k: fit[k] for k in K.FIT} == K.FIT
    # weight 1 on every pair is the unweighted fit, through the per-entry path
    ones = recs.als_fit(u, i, weight=np.ones(len(u), np.float32), **K.FIT)
    assert torch.equal(ones["X"], fit["X"]) and torch.equal(ones["Y"], fit["Y"])


# ---- lists and ranks --------------------------------------------------------------------------------------------------------
def test_als_topk_and_als_rank_are_rows_topk_and_rows_rank_on_dot_scores():
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
        for batch in (recs.ALS_BATCH, 23):
            got_i, got_s = recs.als_topk(fit, users, 12, watched, batch=batch)
            assert torch.equal(got_i, want_i) and got_s.cpu().numpy().tobytes() == want_s.cpu().numpy().tobytes()
            assert torch.equal(recs.als_rank(fit, users, watched, tr, ta, batch=batch), ops.rows_rank(rows, tr, ta, watched))
    with pytest.raises(ValueError, match="user out of range"):
        recs.als_topk(fit, [0, n_users], 5)
    with pytest.raises(ValueError, match="target_row out of range"):
        recs.als_rank(fit, users, None, [70], [0])


# ---- planted blocks -----------------------------------------------------------------------------------------------------
def test_planted_blocks_als_ranks_the_held_out_pairs_above_popularity():
    """tests/test_als_cpu.py shows the gap on the fp64 restatement first: mean ranks 6.4 (ALS) and 15.5 (popularity)."""
    from anime_recommendations_amd import ops, recs
    tu, ti, hu, hi = K.block_pairs()
    fit = recs.als_fit(tu, ti, **K.BLOCK)
    seen = recs.listed_seen_bits(tu, ti, hu, K.BLOCK["n_users"], K.BLOCK["n_items"])
    als_rank = recs.als_rank(fit, hu, seen, np.arange(len(hu)), hi).cpu().numpy()
    pop = recs.popularity_scores(ti, K.BLOCK["n_items"], K.BLOCK["n_users"]).to(DEV)
    pop_rank = ops.score_rank(pop, len(hu), np.arange(len(hu)), hi, watched_bits=seen).cpu().numpy()
    print("planted blocks: mean rank ALS %.2f, popularity %.2f" % (als_rank.mean(), pop_rank.mean()))
    assert als_rank.mean() < pop_rank.mean()
    # the GPU ranks are the restatement's ranking rule on the GPU's own scores
    scores = (fit["X"].double() @ fit["Y"].double().T).cpu().numpy()
    assert abs(K.mean_rank(scores, tu, ti, hu, hi) - als_rank.mean()) <= 0.5


# ---- evaluate ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recs_table(tmp_path_factory):
    from anime_recommendations_amd import components as C, data, weights_io
    work = tmp_path_factory.mktemp("als")
    rec = RF.load()
    z, df = rec["npz"], RF.ratings(rec)
    user_ids, anime_ids = C.index_tables({}, df)
    pq, mp = str(work / "user_stats.parquet"), str(work / "wandb_anime_nn.h5")
    df.to_parquet(pq, index=False)
    weights_io.save_model(mp, z["U"], z["A"], dict(rec["model_recs"]["heads"]["sigmoid"], activation="sigmoid"),
                          user_ids=user_ids, anime_ids=anime_ids)
    return weights_io.load_model(mp), data.load_user_stats(pq)


def test_evaluate_frame_baseline_als_on_the_recs_fixture(recs_table):
    from anime_recommendations_amd import components as C, recs
    model, table = recs_table
    ks, par = [1, 5, 20], dict(factors=32, sweeps=2, cg_steps=2, alpha=4.0, reg=0.05, min_rating=0.6, seed=3)
    plain_frame, plain = C.evaluate_frame(model, table, 1000, ks, 0.7)
    none_frame, none = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline=None, als=par)
    assert none_frame.to_csv(index=False) == plain_frame.to_csv(index=False) and none == plain
    assert plain_frame.columns.tolist() == ["k", "hit_rate", "ndcg"]
    assert list(plain) == ["n", "n_users", "test_size", "min_rating", "mrr", "mean_rank", "median_rank"] + \
        [f % k for k in ks for f in ("hit_rate@%d", "ndcg@%d")]
    frame, summary = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline=["als", "popularity"], als=par)
    assert frame.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity", "hit_rate_als",
                                      "ndcg_als"]
    assert list(summary)[-8:] == ["als_mrr", "als_mean_rank"] + \
        ["als_%s@%d" % (f, k) for k in ks for f in ("hit_rate", "ndcg")]
    assert frame[["k", "hit_rate", "ndcg"]].to_csv(index=False) == plain_frame.to_csv(index=False)
    # the als columns are a direct fit and rank with the same parameters
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    assert len(row) > 100
    tu, ta, tr = (np.asarray(c[train]) for c in (table.user, table.anime, table.rating))
    liked = tr.astype(np.float32) >= np.float32(0.6)
    fit = recs.als_fit(tu[liked], ta[liked], table.n_users, table.n_anime, 32, 2, 2, 4.0, 0.05, seed=3)
    seen = recs.listed_seen_bits(tu, ta, users, table.n_users, table.n_anime)
    b = recs.ranking_metrics(recs.als_rank(fit, users, seen, row, anime), ks)
    assert frame["hit_rate_als"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_als"].tolist() == [b["ndcg"][k] for k in ks]
    assert summary["als_mrr"] == b["mrr"] and summary["als_mean_rank"] == b["mean_rank"]
    # with the bootstrap the als system has its intervals and the model its paired differences against it
    ci_frame, ci = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline="als", als=par, ci_replicates=50, ci_seed=1)
    for col in ("hit_rate_als_lo", "hit_rate_als_hi", "ndcg_als_lo", "ndcg_als_hi", "hit_rate_diff_als",
                "hit_rate_diff_als_lo", "hit_rate_diff_als_hi", "hit_rate_p_als", "ndcg_diff_als", "ndcg_p_als"):
        assert col in ci_frame.columns, col
    for key in ("als_mrr_lo", "als_mrr_hi", "als_mean_rank_lo", "als_mean_rank_hi", "mrr_diff_als", "mrr_p_als",
                "mean_rank_diff_als_lo", "mean_rank_diff_als_hi"):
        assert key in ci, key
    assert ci_frame["hit_rate_als"].tolist() == frame["hit_rate_als"].tolist()
    assert (ci_frame["hit_rate_als_lo"] <= ci_frame["hit_rate_als"]).all() and \
        (ci_frame["hit_rate_als"] <= ci_frame["hit_rate_als_hi"]).all()
    assert ci["als_mrr_lo"] <= ci["als_mrr"] <= ci["als_mrr_hi"]
    with pytest.raises(ValueError, match="32, 64, 128, 256"):
        C.evaluate_frame(model, table, 1000, ks, 0.7, baseline="als", als=dict(par, factors=48))
