"""GPU tests of the capped and split launches (DESIGN.md "Launch caps"): every entry point that caps its grid and lets the
workgroups stride over the rest, or cuts a call into several launches, run JUST PAST the cap — the second pass of the
strided loop, the second launch with its shifted pointers — at the smallest shape that gets there.

Yardsticks: the NumPy restatements the entry points' own test files use (bpr, kmeans, cooc, rp3, tsne, boot), pandas for
the ingest path.  Every comparison is bit for bit or on exact integers; no tolerance is used anywhere.  The shapes, the
inputs and the references live in tests/launch_caps_cases.py; tests/test_launch_caps_cpu.py holds each shape against the
cap in the kernel's source, so these cases cannot silently fall back to one pass.
"""
import numpy as np
import pandas as pd
import pytest
import torch

import boot_restatement as BR
import cooc_restatement as CO
import cover_restatement as CV
import ease_restatement as ER
import favourites_restatement as FV
import kmeans_restatement as K
import launch_caps_cases as L
import poison
from oracle import anirec_oracle as anirec_orc
from oracle import ingest_oracle as orc
from test_boot_gpu import _case as _boot_case
from test_bpr_gpu import _same, _steps
from test_cover_gpu import _dirty, _greedy, _invariants, _rated, _same as _same_cover
from test_favourites_gpu import _run as _favourites, _same as _same_favourites
from test_ingest_gpu import _check, _raw_frame
from test_kmeans_gpu import _same_fit as _same_kmeans_fit, _sims_fn
from test_mmr_gpu import _bits, _cuda
from test_tsne_gpu import _same_fit as _same_tsne_fit, _same_forces

pytestmark = pytest.mark.gpu
NAN_BITS = np.uint32(0x7FC00000)
POISON = 0x7F
POISON_I32 = 0x7F7F7F7F


# ---- BPR ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,batch", L.BPR_CASES)
def test_bpr_steps_past_the_block_cap(width, batch):
    """k_bpr_grad / k_bpr_apply: 4096 workgroups of 1024 / width slots; three passes at width 256, two at 32 and 128"""
    p = L.BPR_STEPS
    assert L.passes(batch, L.bpr_pass_slots(width)) >= 2
    X, Y = L.bpr_tables(width)
    gx, gy, gc, ge = _steps(X, Y, L.bpr_lists(), batch, p["tries"], p["seed"], p["step0"], p["n_steps"], p["lr"], p["reg"],
                            p["bias"])
    wx, wy, wc, we = L.bpr_ref(width, batch)
    assert ge == we == 0
    assert _same(gc, wc), (gc, wc)
    assert _same(gx, wx) and _same(gy, wy), (int((gx != wx).any(axis=1).sum()), int((gy != wy).any(axis=1).sum()))
    for step in range(p["n_steps"]):                             # the count exchange ACROSS passes is exercised
        kept, slots, touches = L.bpr_shared_rows(width, batch, step)
        assert touches > 1 and (slots > 1 or kept == 1), (step, kept, slots, touches)


def test_bpr_steps_rows_that_only_the_later_pass_updates():
    """width 64, 65 536 + 300 slots on 200 000 users of one to three items: in the cases above the first-pass winner of
    a row's count applies the whole sum, so k_bpr_apply's later passes find every count taken; here more than 100 user
    rows are touched by slots of the second pass alone, and their update is that pass's"""
    p = L.BPR_SPARSE
    X, Y = L.bpr_sparse_tables()
    gx, gy, gc, ge = _steps(X, Y, L.bpr_sparse_lists(), p["batch"], p["tries"], p["seed"], p["step0"], p["n_steps"], p["lr"],
                            p["reg"], p["bias"])
    wx, wy, wc, we, own = L.bpr_sparse_ref()
    assert ge == we == 0 and _same(gc, wc), (gc, wc)
    assert _same(gx[own], wx[own]), int((gx[own] != wx[own]).any(axis=1).sum())
    assert _same(gx, wx) and _same(gy, wy), (int((gx != wx).any(axis=1).sum()), int((gy != wy).any(axis=1).sum()))
    assert len(own) > 100 and (wx[own] != X[own]).any(axis=1).all()


def test_bpr_sample_past_the_block_cap():
    """k_bpr_sample: 65 536 workgroups of 256 entries; 17 steps of 2^20 slots, the last one wholly in the second pass"""
    from anime_recommendations_amd import ops
    p = L.SAMPLE
    total = p["n_steps"] * p["batch"]
    assert L.passes(total, L.sample_pass_entries()) == 2
    log = []
    with poison.poisoned(POISON, log):
        out = ops.bpr_sample(*L.bpr_lists(), L.BPR_ITEMS, p["batch"], p["tries"], p["seed"], p["step0"], p["n_steps"])
    assert max(log) == total * 12 and tuple(out.shape) == (p["n_steps"], p["batch"], 3)
    for step in L.SAMPLE_CHECKED:
        got, want = out[step].cpu().numpy(), L.sample_ref(step)
        assert _same(got, want), (step, int((got != want).any(axis=1).sum()))
    assert not bool((out == POISON_I32).any())                   # every entry of every step was written


# ---- k-means ------------------------------------------------------------------------------------------------------
def _km_table(case):
    """the unit rows of the case on the device: N(0, 1) rows normalised, then an unusable row (one NaN element) and a
    pair of bit-identical rows planted inside the second pass"""
    from anime_recommendations_amd import ops
    g = torch.Generator(device="cuda")
    g.manual_seed(1000 + case["dim"])
    Wh = ops.rownorm(torch.randn(case["n_rows"], case["dim"], generator=g, device="cuda"))
    bad, ta, tb = L.km_planted(case)
    Wh[tb] = Wh[ta]
    Wh[bad, 3] = float("nan")
    return Wh


@pytest.fixture(scope="module")
def km_table_a():
    """case A's table, shared by the assign and the fit case (neither writes it) and freed with the module"""
    return _km_table(L.KM_A)


def _km_centroids(case):
    rng = np.random.default_rng(600 + case["dim"])
    C = rng.normal(size=(case["k"], case["dim"]))
    return (C / np.linalg.norm(C, axis=1, keepdims=True)).astype(np.float32)


def _planted_did_their_work(case, rows, ra, rs):
    """on the reference, at the positions ``rows`` (row -> position) holds"""
    bad, ta, tb = (rows[r] for r in L.km_planted(case))
    assert ra[bad] == -1 and _bits(rs[bad]) == NAN_BITS
    assert ra[ta] == ra[tb] >= 0 and _bits(rs[ta]) == _bits(rs[tb])


def test_kmeans_assign_past_the_grid_cap_one_tile(km_table_a):
    """case A: width 32, k = 3, 262 144 + 300 rows: the image is staged once and REUSED on the second batch"""
    from anime_recommendations_amd import ops
    case = L.KM_A
    Wh, C = km_table_a, _km_centroids(case)
    a, s = ops.kmeans_assign(Wh, _cuda(C))
    ra, rs = K.assign(_sims_fn(Wh)(C), K.usable(Wh.cpu().numpy()))
    a, s = a.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(a, ra), np.flatnonzero(a != ra)[:10]
    assert np.array_equal(_bits(s), _bits(rs)), np.flatnonzero(_bits(s) != _bits(rs))[:10]
    _planted_did_their_work(case, {r: r for r in L.km_planted(case)}, ra, rs)
    assert len(np.unique(ra[L.km_pass_rows(32):])) == 4         # the second pass picks every centroid, and -1


def test_kmeans_assign_past_the_grid_cap_two_tiles():
    """case B: width 256 (two lanes a row), k = tile + 1, 131 072 + 129 rows: the image is RESTAGED on the second batch.
    A row's pick depends on that row and C alone, so the oracle is computed for the rows of the second pass, the 256 on
    each side of the pass boundary and 1000 others, as a table of their own."""
    from anime_recommendations_amd import ops
    case = L.KM_B
    first, n = L.km_pass_rows(case["dim"]), case["n_rows"]
    Wh, C = _km_table(case), _km_centroids(case)
    a, s = ops.kmeans_assign(Wh, _cuda(C))
    others = np.random.default_rng(3).choice(first - 256, 1000, replace=False)
    rows = np.unique(np.concatenate([np.arange(first - 256, n), others]))
    assert len(rows) == 256 + (n - first) + 1000 and first + 256 >= n
    sub = Wh[_cuda(rows)].contiguous()
    ra, rs = K.assign(_sims_fn(sub)(C), K.usable(sub.cpu().numpy()))
    a, s = a.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(a[rows], ra), rows[a[rows] != ra][:10]
    assert np.array_equal(_bits(s[rows]), _bits(rs)), rows[_bits(s[rows]) != _bits(rs)][:10]
    _planted_did_their_work(case, {int(r): i for i, r in enumerate(rows)}, ra, rs)
    assert (ra >= L.km_tile(case["dim"])).any()                  # the centroid of the second tile is picked somewhere
    assert (a[np.setdiff1d(np.arange(n), [L.km_planted(case)[0]])] >= 0).all() and a.max() < case["k"]


def test_kmeans_fit_past_the_grid_cap(km_table_a):
    """width 32, k = 3, 262 144 + 300 rows, two iterations against the restatement's fit in full; outputs and workspace
    filled with 0x7F first, so k_kmeans_init's stride (a_0 = -2, the workspace to zero) and k_kmeans_count's are held
    beside the assign kernel's"""
    from anime_recommendations_amd import ops
    case = L.KM_A
    Wh = km_table_a
    Wh_host = Wh.cpu().numpy()
    C0 = Wh[:case["k"]].clone()
    ref = K.fit(Wh_host, Wh_host[:case["k"]], L.KM_FIT_ITERS, _sims_fn(Wh))
    log = []
    with poison.poisoned(POISON, log):
        got = ops.kmeans_fit(Wh, C0, L.KM_FIT_ITERS)
    assert len(log) == 5 and max(log) == case["n_rows"] * 4     # assign, sim, count, info, workspace
    _same_kmeans_fit(got, ref, "fit")
    rC, ra, rs, rcount, rinfo = ref
    assert tuple(rinfo) == (L.KM_FIT_ITERS, 0) and rcount.sum() == case["n_rows"] - 1 and rcount.min() > 1000
    _planted_did_their_work(case, {r: r for r in L.km_planted(case)}, ra, rs)


def test_rownorm_past_the_block_cap():
    """k_rownorm: 4096 workgroups of 1024 / width rows.  A row's result depends on that row alone, so the rows of a
    strided call equal, bit for bit, the same rows normalised in calls below the cap; and the rows of the second pass
    and the 1000 before it are held to NumPy at test_width_gpu's bar for this kernel (2 ulp: the order of the sum)."""
    from anime_recommendations_amd import ops
    for dim in L.ROWNORM_WIDTHS:
        per = L.rownorm_pass_rows(dim)
        n = per + 37
        g = torch.Generator(device="cuda")
        g.manual_seed(dim)
        W = torch.randn(n, dim, generator=g, device="cuda")
        W[per + 5] = 0
        with poison.poisoned(POISON, []):
            got = ops.rownorm(W)
        want = torch.cat([ops.rownorm(W[:per - 1].contiguous()), ops.rownorm(W[per - 1:].contiguous())])
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), dim
        assert bool(torch.isnan(got[per + 5]).all()) and not bool(torch.isnan(got[per + 6:]).any())
        tail, host = got[per - 1000:].cpu().numpy(), W[per - 1000:].cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = host / np.linalg.norm(host, axis=1).reshape(-1, 1)
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(tail), ~ok) and ok.sum() == (1000 + 36) * dim
        assert np.all(np.abs(tail[ok] - ref[ok]) <= 2 * np.spacing(np.abs(ref[ok]).astype(np.float32))), dim


# ---- co-occurrence ------------------------------------------------------------------------------------------------
def _rows_equal(got, want6, row, what):
    """``got`` [nq, m] on the device equals ``want6[row]`` bit for bit; the tiles on both sides of the launch boundary and
    the last tile are asserted on their own first: a mis-shifted pointer shows there"""
    want6 = torch.from_numpy(np.ascontiguousarray(want6)).cuda()
    if want6.dtype.is_floating_point:
        got, want6 = got.view(torch.int32), want6.view(torch.int32)
    last = (L.COOC["nq"] - 1) // L.caps()["cooc_tile"]
    for tile in (L.caps()["cooc_tiles"] - 1, L.caps()["cooc_tiles"], last):
        r = L.cooc_tile_rows(tile)
        assert torch.equal(got[r], want6[row[r]]), (what, "tile", tile)
    assert torch.equal(got, want6[row]), what


def test_cooc_scores_second_launch():
    """anirec_cooc_scores: launches of 32 768 tiles of 64 queries; 32 768 * 64 + 70 queries make a second launch of two
    tiles, the last one partial, with the one bad query in it"""
    from anime_recommendations_amd import ops
    p = L.COOC
    bits, queries, row, _, _, _ = L.cooc_inputs()
    wsim, wcnt, wexcl, wpop, werr = L.cooc_ref()
    row = _cuda(row)
    with poison.poisoned(POISON, []):
        sim, cnt, excl, pop, err = ops.cooc_scores(_cuda(bits.view(np.int32)), p["n_users"], _cuda(queries), p["measure"],
                                                   p["shrink"], p["min_support"], count=True, excl=True, pop=True, check=False)
    assert int(err.item()) == werr == 1
    assert np.array_equal(pop.cpu().numpy(), wpop)
    _rows_equal(sim, wsim, row, "sim")
    _rows_equal(cnt, wcnt, row, "count")
    _rows_equal(excl, wexcl.view(np.int32), row, "excl")
    bad = L.COOC_BAD_AT                                          # as the restatement says: NaN, -1, all excluded
    assert bool(torch.isnan(sim[bad]).all()) and bool((cnt[bad] == -1).all()) and int(excl[bad, 0]) == (1 << p["n_items"]) - 1
    assert not bool(torch.isnan(sim[bad + 1:]).any()) and not bool(torch.isnan(sim[:bad]).any())


def test_wcooc_scores_second_launch():
    """anirec_wcooc_scores: the same split on the i8 matrix-core kernel, with the sums and the excl words asked for"""
    from anime_recommendations_amd import ops
    p = L.COOC
    bits, queries, row, user_q, rs, cs = L.cooc_inputs()
    ww, wsum, wexcl, werr = L.wcooc_ref()
    row = _cuda(row)
    with poison.poisoned(POISON, []):
        w, sm, excl, err = ops.wcooc_scores(_cuda(bits.view(np.int32)), p["n_users"], user_q, _cuda(queries), rs, cs,
                                            sums=True, excl=True, check=False)
    assert int(err.item()) == werr == 1
    _rows_equal(w, ww, row, "w")
    _rows_equal(sm, wsum, row, "sum")
    _rows_equal(excl, wexcl.view(np.int32), row, "excl")
    bad = L.COOC_BAD_AT
    assert bool(torch.isnan(w[bad]).all()) and bool((sm[bad] == -1).all()) and int(excl[bad, 0]) == (1 << p["n_items"]) - 1
    assert not bool(torch.isnan(w[bad + 1:]).any()) and not bool(torch.isnan(w[:bad]).any())


# ---- t-SNE --------------------------------------------------------------------------------------------------------
def _tsne_dev():
    Y, offsets, idx, val, _, _ = L.tsne_case()
    return _cuda(Y), _cuda(offsets), _cuda(idx), _cuda(val)


def test_tsne_forces_past_the_init_cap():
    """k_tsne_init: 1024 workgroups of 256 words; 262 144 + 200 rows, outputs filled with 0x7F first.  The oracle is
    known without an all-pairs pass in NumPy (launch_caps_cases.tsne_case): all rows but 50 sit on a lattice so coarse
    that every pair term with a lattice point quantises to exactly 0; the 50, at rows past the first pass, carry the
    restatement's sums of the 50 alone."""
    from anime_recommendations_amd import ops
    log = []
    with poison.poisoned(POISON, log):
        got = ops.tsne_forces(*_tsne_dev())
    assert log.count(L.TSNE["n"] * 8) == 4                       # rx, ry, ax, ay
    _same_forces(got, L.tsne_forces_ref(), "forces")


@pytest.mark.parametrize("iters", L.TSNE_ITERS)
def test_tsne_fit_past_the_init_cap(iters):
    """odd iteration counts: the init kernel also copies Y into the second buffer, strided; V, G and the workspace start
    as 0x7F bytes.  Every lattice row: Y as it was, V = 0, G = 0.8^iters by the restatement's update of a zero gradient"""
    from anime_recommendations_amd import ops
    p = L.TSNE
    d = _tsne_dev()
    want = L.tsne_fit_ref(iters)
    with poison.poisoned(POISON, []):
        Y, V, G, info = ops.tsne_fit(*d, iters, p["exag_iters"], p["exaggeration"], p["lr"])
    _same_tsne_fit((Y, V, G, info), want, iters)
    Y0, rows = L.tsne_case()[0], L.tsne_case()[4]
    lattice = np.setdiff1d(np.arange(p["n"]), rows)
    Y, V, G = Y.cpu().numpy(), V.cpu().numpy(), G.cpu().numpy()
    assert np.array_equal(_bits(Y[lattice]), _bits(Y0[lattice])) and (V[lattice].view(np.uint64) == 0).all()
    assert (G[lattice] == want[2][lattice[0], 0]).all() and (iters != 1 or want[2][lattice[0], 0] == 0.8)
    assert np.array_equal(d[0].cpu().numpy(), Y0)                # Y0 is not modified


# ---- ingest -------------------------------------------------------------------------------------------------------
def test_ingest_preprocess_past_the_minmax_and_init_caps():
    """600 000 ungrouped rows with drop_half_watched: k_ing_minmax (2048 workgroups of 256 rows) strides; the user ids
    spread past 524 288, so k_ing_init's fill of the per-user tables strides too.  Against pandas, bit for bit."""
    first = L.caps()["ing_minmax_blocks"] * 256
    df = _raw_frame(L.INGEST_ROWS, 900, 700, seed=41)
    df["user_id"] = df["user_id"] * L.INGEST_USER_SCALE
    df.loc[:first - 1, "rating"] = df.loc[:first - 1, "rating"].clip(1, 9)     # the extremes live in the second pass only
    assert df["user_id"].max() > first and set(df["rating"][:first].dropna()) == set(range(1, 10))
    with poison.poisoned(POISON, []):                            # outputs and workspace: what k_ing_init must fill is dirty
        want = _check(df, 150, drop_half_watched=True)
    assert 100_000 < len(want) < len(df) and want["user_id"].max() > first
    raw = df["rating"][want.index]                               # the oracle keeps the frame's index
    assert raw[raw == 0].index.min() >= first and raw[raw == 10].index.min() >= first       # survivors of the second pass
    assert (want["rating"][raw == 0] == 0.0).all() and (want["rating"][raw == 10] == 1.0).all()      # scaled by 0 and 10


def test_ingest_preprocess_past_the_list_cap():
    """k_nl_insert / k_nl_count / k_nl_filter: 4096 workgroups of 256 list entries.  In a frame that is not grouped by
    user every complete row goes through the list, so 1 150 000 rows make a second pass (and k_nl_clear four)."""
    df = _raw_frame(L.INGEST_LIST_ROWS, 900, 700, seed=45)
    assert df.notna().all(axis=1).sum() > L.caps()["ing_list_blocks"] * 256
    with poison.poisoned(POISON, []):                            # the list's hash table starts dirty: k_nl_clear fills it
        want = _check(df, 300)
    assert 500_000 < len(want) < len(df)


def test_ingest_encode_past_the_init_cap():
    """600 000 ids below 600 001: k_enc_init's fill of the first-row table strides.  Against ``Series.unique()``."""
    from anime_recommendations_amd import ingest
    ids = np.random.default_rng(43).integers(0, L.INGEST_ENCODE_IDS, L.INGEST_ROWS).astype(np.int32) * 3 + 1
    ids[-1] = 3 * L.INGEST_ENCODE_IDS - 2                         # the largest id: the table's last word
    with poison.poisoned(POISON, []):                            # the first-row table and the bit words start dirty
        idx, uniq = ingest.encode_ids(torch.as_tensor(ids, device="cuda"))
    want_idx, want_uniq = orc.encode(pd.Series(ids))
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(uniq.cpu().numpy(), want_uniq)


def test_ingest_id_max_past_the_block_cap():
    """k_ing_id_max: 2048 workgroups of 4096 rows a pass (256 lanes, four quads of four rows each); 2048 * 4096 + 7
    rows, the two maxima in the 7 rows of the second pass, a NULL among them"""
    from anime_recommendations_amd import ops
    n = L.ID_MAX_ROWS
    rng = np.random.default_rng(47)
    u = rng.integers(0, 1_000_000, n).astype(np.int32)
    a = rng.integers(0, 1_000_000, n).astype(np.int32)
    u[n - 7], a[n - 1], a[n - 2] = 1_000_003, 1_000_001, -(2 ** 31)
    mx = poison.fill(torch.empty(2, dtype=torch.int32, device="cuda"), POISON)
    ops._call("anirec_ingest_id_max", _cuda(u), _cuda(a), n, mx)
    assert mx.tolist() == [int(u.max()), int(a.max())] == [1_000_003, 1_000_001]
    u[n - 7], a[n - 1] = 5, 5                                    # without the tail's maxima: the first pass's
    ops._call("anirec_ingest_id_max", _cuda(u), _cuda(a), n, mx)
    assert mx.tolist() == [int(u.max()), int(a.max())]


# ---- the flat optimiser steps and the rating gather ---------------------------------------------------------------
def test_adam_flat_and_opt_flat_past_the_block_cap():
    """k_adam_flat / k_opt_flat: 4096 workgroups of 256 elements; 77 elements more, bit for bit against the oracle's
    element rules as test_train_gpu and test_optimizers_gpu hold them below the cap"""
    from anime_recommendations_amd import ops
    n = L.FLAT_ELEMS
    rng = np.random.default_rng(61)
    w0 = rng.normal(0, 0.05, n).astype(np.float32)
    g = rng.normal(0, 1e-4, n).astype(np.float32)
    g[-77:] *= 100                                               # steps well above an ulp of w in the second pass
    g[-50:-40] = 0
    w, m, v = w0.copy(), rng.normal(0, 1e-5, n).astype(np.float32), (rng.normal(0, 1e-5, n) ** 2).astype(np.float32)
    alpha = anirec_orc.adam_alpha(4.2e-5, 1234)
    tw, tm, tv, tg = (_cuda(x.copy()) for x in (w, m, v, g))
    ops.adam_flat(tw, tm, tv, tg, alpha)
    anirec_orc.adam_update(w, m, v, g, alpha)
    for got, want in ((tw, w), (tm, m), (tv, v)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert (w[-77:] != w0[-77:]).sum() > 60                      # the second pass moved its elements
    for kind in anirec_orc.KINDS:
        w = w0.copy()
        s = (rng.random(n) * 1e-6).astype(np.float32) + np.float32(anirec_orc.SLOT_INIT[kind])
        tw, ts = _cuda(w.copy()), _cuda(s.copy())
        ops.opt_flat(kind, tw, None if kind == "sgd" else ts, tg, np.float32(4.2e-5))
        anirec_orc.opt_update(kind, w, None, s, g, np.float32(4.2e-5))
        assert np.array_equal(_bits(tw.cpu().numpy()), _bits(w)), kind
        assert kind == "sgd" or np.array_equal(_bits(ts.cpu().numpy()), _bits(s)), kind
        assert (w[-77:] != w0[-77:]).sum() > 60, kind


def test_gather_ratings_past_the_block_cap():
    """k_gather_ratings: 8192 workgroups of 256 rows; 33 rows more, against NumPy's take"""
    from anime_recommendations_amd import ops
    n = L.GATHER_ROWS
    rng = np.random.default_rng(67)
    u, a = rng.integers(0, 350_000, n).astype(np.int32), rng.integers(0, 18_000, n).astype(np.int32)
    t = rng.random(n).astype(np.float32)
    perm = rng.permutation(n)
    with poison.poisoned(POISON, []):
        uo, ao, to = ops.gather_ratings(_cuda(u), _cuda(a), _cuda(t), _cuda(perm))
    assert np.array_equal(uo.cpu().numpy(), u[perm]) and np.array_equal(ao.cpu().numpy(), a[perm])
    assert np.array_equal(_bits(to.cpu().numpy()), _bits(t[perm]))


# ---- bootstrap ----------------------------------------------------------------------------------------------------
def test_boot_weights_past_the_block_cap():
    """k_boot_weights: 65 536 workgroups of 256 entries; 4096 replicates of 4097 units are 4096 entries more"""
    from anime_recommendations_amd import ops
    n_units, n_rep = L.BOOT_WEIGHTS["n_units"], L.BOOT_WEIGHTS["n_rep"]
    assert L.passes(n_units * n_rep, L.caps()["boot_blocks"] * 256) == 2
    keys = np.random.default_rng(53).integers(-(1 << 31), 1 << 31, n_units, dtype=np.int64).astype(np.int32)
    thr = BR.poisson1_thresholds()
    with poison.poisoned(POISON, []):
        got = ops.boot_weights(_cuda(keys), 12345, n_rep, thr)
    want = BR.boot_weights(keys, 12345, n_rep, thr)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n_rep, n_units)
    assert torch.equal(got, _cuda(want)), int((got.cpu() != torch.from_numpy(want)).sum())


def test_boot_sums_past_the_unit_splits_and_the_combine_cap():
    """k_boot_partial: split y takes every gridDim.y-th unit tile.  16 383 replicates of 25 columns make 8 splits, and
    1224 units 10 tiles: splits 0 and 1 take a second tile, the last one partial.  k_boot_combine: 65 536 workgroups of
    256 cells; 65 537 rows of 256 columns are 256 cells more (three units keep the oracle cheap)."""
    from anime_recommendations_amd import ops
    thr = BR.poisson1_thresholds()
    for case in (L.BOOT_SPLITS, L.BOOT_COMBINE):
        values, keys = _boot_case(case["n_units"], case["n_col"], 59)
        with poison.poisoned(POISON, []):
            out, err = ops.boot_sums(_cuda(values), _cuda(keys), 7, case["n_rep"], thr, check=False)
        want, werr = BR.boot_sums(values, keys, 7, case["n_rep"], thr)
        assert int(err.item()) == werr == 0 and tuple(out.shape) == want.shape
        assert torch.equal(out, _cuda(want)), (case, int((out.cpu() != torch.from_numpy(want)).sum()))


# ---- onboarding lists, EASE weights ---------------------------------------------------------------------------------
def test_cover_greedy_past_the_group_cap():
    """k_cover_gain: 768 workgroups of 8 rows (a wave a row); 9 items more, one of them rated by everyone, so the first
    pick comes out of the second pass and the later ones are held against it"""
    first, n_items, n_users = L.cover_pass_items(), L.COVER_ITEMS, 70
    M = _rated(n_items, n_users, 0.3, 71)
    M[first + 3] = True
    clean = CO.pack_bits(M)
    bits = _dirty(clean, n_users, 3)
    rng = np.random.default_rng(73)
    P = rng.random(n_users) < 0.6
    open_bits = _dirty(CO.pack_bits(P[None]), n_users, 5)[0]
    keep = (rng.random(n_items) < 0.8).astype(np.uint8)
    keep[first + 3] = 1
    for m, depth in ((7, 2), (10, 1)):
        got = _greedy(bits, n_users, m, depth, open_bits, keep)
        _same_cover(got, CV.cover_greedy(clean, n_users, m, depth, open_bits, keep)[:3], (m, depth))
        _invariants(M, P, *got, depth, (m, depth))
        assert got[0][0] == first + 3 and got[1][0] == P.sum()


def test_ease_weights_past_the_row_cap():
    """k_ease_weights: grid.y = min(n, 1024) row walkers; 1024 + 5 rows.  One fp64 divide and one rounding an element:
    bit for bit against the restatement on the same P"""
    from anime_recommendations_amd import ops
    n = L.EASE_ROWS
    rng = np.random.default_rng(79)
    P = rng.normal(size=(n, n))
    P[np.diag_indices(n)] = rng.random(n) + 0.5
    with poison.poisoned(POISON, []):
        W = ops.ease_weights(_cuda(P))
    assert np.array_equal(_bits(W.cpu().numpy()), _bits(ER.ease_weights(P)))


# ---- the any-k select's merge, the favourites' scatter ---------------------------------------------------------------
def test_rows_topk_past_the_merge_cap():
    """k_lk_merge: 4096 workgroups of 256 entries a query; one row of 1 048 576 + 4099 scores and k = n, so every merge
    pass and the last one (which writes the output row) take a second pass.  Against the restatement's stable sort."""
    from anime_recommendations_amd import ops
    n = L.MERGE_COLS
    rng = np.random.default_rng(83)
    scores = rng.normal(size=(1, n)).astype(np.float32)
    scores[0, -4099:] += 3                                       # the head of the list comes out of the last columns
    scores[0, rng.integers(0, n, 1000)] = np.float32(0.25)      # ties: by index
    scores[0, 5], scores[0, n - 2] = np.nan, np.nan
    with poison.poisoned(POISON, []):
        gi, gs = ops.rows_topk(_cuda(scores), n)
    wi, ws = CO.rows_topk(scores, n)
    assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(_bits(gs.cpu().numpy()), _bits(ws))
    assert wi[0, 0] >= n - 4099 and sorted(wi[0, -2:].tolist()) == [5, n - 2]


def test_user_favourites_past_the_scatter_cap():
    """k_rec_scatter: 16 384 workgroups of 256 ratings, run for a table that is not grouped by user; 4 194 304 + 4099
    shuffled ratings of 100 000 users against the restatement test_favourites_cpu holds to the oracle"""
    n_users, n_anime = 100_000, 64
    table = FV._few_ratings(np.random.default_rng(89), np.arange(n_users), n_anime, 40, 48, grid=True)
    assert len(table[0]) > L.SCATTER_ROWS
    table = FV.shuffled(tuple(c[:L.SCATTER_ROWS] for c in table), 7)
    with poison.poisoned(POISON, []):
        got = _favourites(table, n_users, n_anime)
    _same_favourites(got, FV.favourites(*table, n_users, n_anime), "shuffled")
