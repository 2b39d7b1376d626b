"""GPU tests of the mapped tables (anirec_tsne_forces / anirec_tsne_fit, ops.tsne_forces / tsne_fit, recs.map_affinities /
map_rows / map_place, components.map_frame, the embedding_map component).

Yardstick: the NumPy restatement (tests/tsne_restatement.py).  Every comparison of the integer sums, of Z's two words, of
Y, V, G and of the info bits is exact, on bits.  A reference is computed once per graph (50 iterations, with the states
after 1, 2, 5 and 50 kept) and shared.

Graphs: n random points (N(0, 1) * 2, fp32) under a random symmetric graph of about 16 stored pairs a row with P' in
(0, 0.25); from n = 16 on row 0 is a hub with all n - 1 rows stored, rows 5 and 9 are a duplicate pair (the same
coordinates, bit for bit) and row 11 stores nothing (an empty CSR row: it is only repelled).  Sizes around the wave (63, 64, 65), the workgroup
(255, 256, 257) and the LDS tile T = anirec_tsne_tile() (T - 1, T, T + 1 = 1025: more than one tile, more than one
workgroup of rows).

map_affinities' tolerance: the NumPy twin and torch evaluate the same fp64 expressions; their ``exp`` / ``log`` differ by
an ulp or two (2^-52 relative), a row's 64 bisection decisions can then differ only where the entropy lies within such
an error of its target, after which both still close in on the same root: p agrees to about d2 * beta * 2^-50 < 1e-12
relative.  That is far below the spacing of fp32, so the stored fp32 values are equal or, where the fp64 value lies
that close to a rounding boundary, one fp32 ulp apart: the tolerance is 2^-23 relative.  The neighbour lists and with
them offsets and idx are integers and must match exactly.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest

import poison
import tsne_restatement as R
from test_components_gpu import _run, pipeline  # noqa: F401  (the components' pipeline fixture, as it is)
from test_mmr_gpu import N_ROWS, TWIN_A, TWIN_B, ZERO_ROW, _bits, _cuda, _table

pytestmark = pytest.mark.gpu
F32 = np.float32
SNAPS = (1, 2, 5, 50)
EXAG = 3                # the switch of momentum and exaggeration: beyond 1 and 2 iterations, inside 5 and 50
LR = 20.0
HUB, DUP_A, DUP_B, ALONE = 0, 5, 9, 11


def _tile():
    from anime_recommendations_amd import _lib
    return _lib.TSNE_TILE


def _sizes():
    T = _tile()
    return (1, 2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1)


def _graph(n, seed=0):
    """(Y0 fp32 [n, 2], offsets, idx, val) as the module docstring describes"""
    rng = np.random.default_rng(7000 + 13 * n + seed)
    Y = (rng.standard_normal((n, 2)) * 2).astype(F32)
    P = np.triu((rng.random((n, n)) < min(1.0, 8.0 / max(n, 1))) * (rng.random((n, n)) * 0.25), 1)
    if n >= 16:
        P[HUB, 1:] = rng.random(n - 1) * 0.25 + 0.01
        Y[DUP_B] = Y[DUP_A]
    P = P + P.T
    if n >= 16:
        P[ALONE, :] = 0                             # (the storage is not symmetric there: the definition is per stored pair)
    return (Y,) + R.csr_from_dense(P.astype(F32))


_REFS = {}


def _ref(n):
    """the graph of n rows and its restatement fits after 1, 2, 5 and 50 iterations, once"""
    if n not in _REFS:
        g = _graph(n)
        _REFS[n] = (g, R.fit(*g, 50, exag_iters=EXAG, lr=LR, snapshots=SNAPS))
    return _REFS[n]


def _dev(g):
    return _cuda(g[0]), _cuda(g[1]), _cuda(g[2]), _cuda(g[3])


def _same_forces(got, want, what=""):
    rx, ry, ax, ay, z, info = got
    wRx, wRy, wAx, wAy, wZ, winfo = want
    assert info == winfo, (what, info, winfo)
    assert z.cpu().numpy().view(np.uint64).tolist() == R.z_words(wZ).tolist(), what
    for a, b in ((rx, wRx), (ry, wRy), (ax, wAx), (ay, wAy)):
        assert np.array_equal(a.cpu().numpy(), b), what


def _same_fit(got, want, what=""):
    Y, V, G, info = got
    wY, wV, wG, winfo = want
    assert info == winfo, (what, info, winfo)
    assert np.array_equal(_bits(Y.cpu().numpy()), _bits(wY)), what
    assert np.array_equal(V.cpu().numpy().view(np.uint64), wV.view(np.uint64)), what
    assert np.array_equal(G.cpu().numpy().view(np.uint64), wG.view(np.uint64)), what


# ---- the forces pass and the fit against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("n", _sizes())
def test_forces_equal_the_restatement(n):
    from anime_recommendations_amd import ops
    g = _ref(n)[0]
    want = R.forces(*g)
    _same_forces(ops.tsne_forces(*_dev(g)), want, n)
    if n >= 16:     # the planted content did what it is there for (on the reference, which the kernel has just equalled)
        Rx, Ry, Ax, Ay, Z, info = want
        assert g[1][HUB + 1] - g[1][HUB] == n - 1 and g[1][ALONE + 1] == g[1][ALONE]
        assert Ax[ALONE] == 0 and Ay[ALONE] == 0 and (Rx[ALONE] != 0 or Ry[ALONE] != 0)
        assert Rx[DUP_A] == Rx[DUP_B] and Z > 2 * 2 ** 30 and info == 0


@pytest.mark.parametrize("n", _sizes())
def test_fits_of_1_2_5_and_50_iterations_equal_the_restatement(n):
    from anime_recommendations_amd import ops
    g, ref = _ref(n)
    d = _dev(g)
    for iters in SNAPS:
        _same_fit(ops.tsne_fit(*d, iters, EXAG, 12.0, LR), ref[iters], (n, iters))
    assert np.array_equal(d[0].cpu().numpy(), g[0])                         # Y0 is not modified
    if n >= 16:
        assert not np.array_equal(ref[50][0][DUP_A], ref[50][0][DUP_B])     # the duplicates part: their stored pairs differ


@pytest.mark.parametrize("n", (257, 1025))
def test_j_splits_do_not_change_a_bit(n):
    from anime_recommendations_amd import ops
    g, ref = _ref(n)
    d = _dev(g)
    want = R.forces(*g)
    for s in (1, 2, 3, 7):
        _same_forces(ops.tsne_forces(*d, j_splits=s), want, (n, s))
        _same_fit(ops.tsne_fit(*d, 5, EXAG, 12.0, LR, j_splits=s), ref[5], (n, s))
    _same_fit(ops.tsne_fit(*d, 2, EXAG, 12.0, LR, j_splits=1024), ref[2], (n, 1024))     # most ranges empty


@pytest.mark.parametrize("exag", (0, 2, 5, 9))
def test_the_switch_inside_at_and_beyond_iters(exag):
    from anime_recommendations_amd import ops
    g = _ref(257)[0]
    want = R.fit(*g, 5, exag_iters=exag, exaggeration=4.0, lr=LR)
    _same_fit(ops.tsne_fit(*_dev(g), 5, exag, 4.0, LR), want, exag)
    if exag:
        assert not np.array_equal(want[0], R.fit(*g, 5, exag_iters=0, exaggeration=4.0, lr=LR)[0])


# ---- particular inputs -------------------------------------------------------------------------------------------------
def test_z_zero_when_every_point_is_far_from_every_other():
    from anime_recommendations_amd import ops
    n = 70
    Y = (np.stack([np.arange(n) % 9, np.arange(n) // 9], 1) * 50000.0).astype(F32)      # a grid, 50000 > 2^15.5 apart
    g = (Y,) + _graph(n)[1:]
    want = R.forces(*g)
    assert want[4] == 0 and not want[0].any()
    _same_forces(ops.tsne_forces(*_dev(g)), want)
    _same_fit(ops.tsne_fit(*_dev(g), 5, 2, 12.0, LR), R.fit(*g, 5, exag_iters=2, lr=LR))


def test_rows_that_are_out_and_bad_stored_pairs():
    from anime_recommendations_amd import ops
    Y, off, idx, val = (a.copy() for a in _ref(257)[0])
    Y[3] = [np.nan, 1.0]
    Y[64] = [0.5, np.inf]
    Y[200] = [-np.inf, np.nan]
    Y[256] = [2.0 ** 61, 0.0]
    Y[100] = [2.0 ** 60, -2.0 ** 60]               # the largest usable coordinates: in, and every term 0
    want = R.forces(Y, off, idx, val)
    assert want[5] == 1 and not want[0][[3, 64, 200, 256]].any() and not want[2][[3, 64, 200, 256]].any()
    _same_forces(ops.tsne_forces(_cuda(Y), _cuda(off), _cuda(idx), _cuda(val)), want)
    _same_fit(ops.tsne_fit(_cuda(Y), _cuda(off), _cuda(idx), _cuda(val), 5, 2, 12.0, LR),
              R.fit(Y, off, idx, val, 5, exag_iters=2, lr=LR))
    # stored values outside [0, 2], indices outside the table, a stored self pair: 0 each, bits 1 and 2
    Y = _ref(257)[0][0]
    val2, idx2 = val.copy(), idx.copy()
    val2[[4, 300, 700]] = [np.nan, 2.5, -0.1]
    idx2[[900, 1200]] = [257, -1]
    row = int(np.searchsorted(off, 1500, side="right") - 1)
    idx2[1500] = row
    want = R.forces(Y, off, idx2, val2)
    assert want[5] == 6
    _same_forces(ops.tsne_forces(_cuda(Y), _cuda(off), _cuda(idx2), _cuda(val2)), want)
    _same_fit(ops.tsne_fit(_cuda(Y), _cuda(off), _cuda(idx2), _cuda(val2), 3, 1, 12.0, LR),
              R.fit(Y, off, idx2, val2, 3, exag_iters=1, lr=LR))


def test_permuted_rows_give_permuted_bits():
    from anime_recommendations_amd import ops
    n = 257
    (Y, off, idx, val), ref = _ref(n)
    perm = np.random.default_rng(1).permutation(n)          # new row r is old row perm[r]
    inv = np.argsort(perm)
    P = np.zeros((n, n), F32)
    for i in range(n):
        P[i, idx[off[i]:off[i + 1]]] = val[off[i]:off[i + 1]]
    g2 = (Y[perm],) + R.csr_from_dense(P[np.ix_(perm, perm)])
    assert not np.array_equal(g2[2][:20], inv[idx[:20]])    # (the rows' stored pairs are in another order too)
    Y2, V2, G2, info = ops.tsne_fit(*_dev(g2), 5, EXAG, 12.0, LR)
    wY, wV, wG, winfo = ref[5]
    assert info == winfo and np.array_equal(_bits(Y2.cpu().numpy()), _bits(wY[perm]))
    assert np.array_equal(V2.cpu().numpy(), wV[perm]) and np.array_equal(G2.cpu().numpy(), wG[perm])


def test_a_subset_of_the_rows_as_a_call_of_its_own():
    from anime_recommendations_amd import ops
    (Y, off, idx, val), _ = _ref(1025)
    rows = np.sort(np.random.default_rng(2).permutation(1025)[:301])
    P = np.zeros((1025, 1025), F32)
    for i in range(1025):
        P[i, idx[off[i]:off[i + 1]]] = val[off[i]:off[i + 1]]
    g = (Y[rows],) + R.csr_from_dense(P[np.ix_(rows, rows)])
    _same_forces(ops.tsne_forces(*_dev(g)), R.forces(*g))
    _same_fit(ops.tsne_fit(*_dev(g), 5, EXAG, 12.0, LR), R.fit(*g, 5, exag_iters=EXAG, lr=LR))


@pytest.mark.parametrize("byte", poison.ORDER)
def test_poisoned_workspace_and_outputs(byte):
    from anime_recommendations_amd import ops
    g, ref = _ref(257)
    d = _dev(g)
    log = []
    with poison.poisoned(byte, log):
        got = ops.tsne_forces(*d)
    assert len(log) >= 6
    _same_forces(got, R.forces(*g), byte)
    for iters in (1, 2):                            # an odd and an even count: both ways through the two Y buffers
        log = []
        with poison.poisoned(byte, log):
            got = ops.tsne_fit(*d, iters, EXAG, 12.0, LR)
        assert len(log) >= 4 and max(log) >= 257 * 24 + iters * 16
        _same_fit(got, ref[iters], (byte, iters))


def test_every_einval_comes_before_a_write():
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    g = _ref(65)[0]
    Y, off, idx, val = _dev(g)
    n, nnz = 65, int(idx.numel())
    mark = 0x5A
    outs = [poison.fill(torch.empty(n * 2, dtype=torch.float64, device="cuda"), mark) for _ in range(6)]
    info = poison.fill(torch.empty(4, dtype=torch.int32, device="cuda"), mark)
    ws = poison.fill(torch.empty(lib.anirec_tsne_workspace_bytes(n, 5), dtype=torch.uint8, device="cuda"), mark)
    Yc = Y.clone()
    D, P = ctypes.c_double, lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def fit(n=n, nnz=nnz, iters=5, exag=2, e=12.0, lr=50.0, s=0, ws_bytes=ws.numel(), wsp=None, **null):
        a = {k: (None if null.get(k) else P(t)) for k, t in
             (("Y", Yc), ("off", off), ("idx", idx), ("val", val), ("V", outs[0]), ("G", outs[1]), ("info", info))}
        return lib.anirec_tsne_fit(a["Y"], n, a["off"], a["idx"], a["val"], nnz, iters, exag, D(e), D(lr), s, a["V"], a["G"],
                                   a["info"], P(ws) if wsp is None else wsp, ws_bytes, None)

    def forces(n=n, nnz=nnz, s=0, **null):
        a = {k: (None if null.get(k) else P(t)) for k, t in
             (("Y", Yc), ("off", off), ("idx", idx), ("val", val), ("rx", outs[2]), ("ry", outs[3]), ("ax", outs[4]),
              ("ay", outs[5]), ("z", outs[0]), ("info", info))}
        return lib.anirec_tsne_forces(a["Y"], n, a["off"], a["idx"], a["val"], nnz, s, a["rx"], a["ry"], a["ax"], a["ay"],
                                      a["z"], a["info"], None)

    for kw in (dict(n=0), dict(n=-1), dict(n=_lib.TSNE_MAX_ROWS + 1), dict(nnz=-1), dict(s=-1), dict(s=1025)):
        assert fit(**kw) == -1 and forces(**kw) == -1, kw
    for kw in (dict(iters=0), dict(iters=4097), dict(exag=-1), dict(e=0.0), dict(e=float("nan")), dict(lr=0.0),
               dict(lr=float("inf")), dict(ws_bytes=ws.numel() - 1), dict(iters=6), dict(wsp=ctypes.c_void_p(ws.data_ptr() + 4)),
               dict(wsp=None, ws_bytes=0), dict(Y=True), dict(off=True), dict(idx=True), dict(val=True), dict(V=True),
               dict(G=True), dict(info=True)):
        assert fit(**kw) == -1, kw
    for name in ("Y", "off", "idx", "val", "rx", "ry", "ax", "ay", "z", "info"):
        assert forces(**{name: True}) == -1, name
    torch.cuda.synchronize()
    for t in outs + [info, ws]:
        assert bool((t.view(torch.uint8) == mark).all())
    assert torch.equal(Yc, Y)
    assert fit() == 0                               # and the same buffers are a good call
    torch.cuda.synchronize()
    assert int(info[0]) == 0 and not torch.equal(Yc, Y)


# ---- one planted case, bit for bit ------------------------------------------------------------------------------------
def test_a_planted_case_of_500_iterations_equals_the_restatement():
    """150 rows x 500 iterations at the default parameters: every bit of Y, V and G.  The purity of this map is the CPU
    suite's (test_tsne_cpu.test_planted_clusters_come_out_pure, case 0: the same inputs)."""
    from anime_recommendations_amd import ops
    clusters, per, D, perp = R.PLANTED[0]
    X, label = R.planted(clusters, per, D, 0)
    n = len(X)
    off, idx, val = R.dense_affinities(X, perp)
    want = R.fit(R.y0(n), off, idx, val, 500, lr=R.auto_lr(n))
    got = ops.tsne_fit(_cuda(R.y0(n)), _cuda(off), _cuda(idx), _cuda(val), 500, 250, 12.0, R.auto_lr(n))
    _same_fit(got, want)
    assert R.knn_purity(got[0].cpu().numpy(), label) == 1.0


# ---- the host layers --------------------------------------------------------------------------------------------------
def _np_neighbours(S, rows, k):
    """the k nearest of ``rows`` to each of them from the score rows S (descending score, ties to the lower row, the row
    itself left out), in the compact numbering of ``rows``"""
    sub = S[np.ix_(rows, rows)].astype(np.float64)
    np.fill_diagonal(sub, -np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(len(rows)), sub.shape), -sub), axis=1)[:, :k]
    return order, np.take_along_axis(S[np.ix_(rows, rows)], order, axis=1)


@pytest.mark.parametrize("dim,perp,k", ((128, 30.0, None), (32, 5.0, 20)))
def test_map_affinities_against_the_numpy_twin(dim, perp, k):
    from anime_recommendations_amd import recs
    Wh, Wh_host, S = _table(dim)
    aff = recs.map_affinities(Wh, perp, k)
    rows = np.flatnonzero(R.usable(Wh_host))
    assert np.array_equal(aff["rows"].cpu().numpy(), rows) and ZERO_ROW not in rows and len(rows) == N_ROWS - 1
    kk = aff["neighbours"]
    assert kk == (90 if k is None else k) and aff["n_rows"] == N_ROWS
    nbr, cos = _np_neighbours(S, rows, kk)
    p, beta = R.conditional_p(2.0 - 2.0 * cos.astype(np.float64), perp)
    off, idx, val = R.symmetrise(nbr, p)
    assert np.array_equal(aff["offsets"].cpu().numpy(), off) and np.array_equal(aff["idx"].cpu().numpy(), idx)
    got = aff["val"].cpu().numpy()
    err = np.abs(got - val) / val
    print("val: %d of %d differ, largest relative difference %.3e" % ((got != val).sum(), len(val), err.max()))
    assert err.max() <= 2.0 ** -23 and np.abs(aff["beta"].cpu().numpy() / beta - 1).max() < 1e-12
    a, b = int(np.flatnonzero(rows == TWIN_A)[0]), int(np.flatnonzero(rows == TWIN_B)[0])
    assert b in idx[off[a]:off[a + 1]] and abs(val.sum() / (2 * len(rows)) - 1) < 1e-5


def test_map_rows_and_map_place():
    import torch
    from anime_recommendations_amd import ops, recs
    Wh, Wh_host, S = _table(64)
    aff = recs.map_affinities(Wh, 20.0)
    fit = recs.map_rows(Wh, 20.0, iters=60, exag_iters=20, seed=4, affinities=aff)
    again = recs.map_rows(Wh, 20.0, iters=60, exag_iters=20, seed=4)
    Y = fit["Y"].cpu().numpy()
    assert np.array_equal(_bits(Y), _bits(again["Y"].cpu().numpy())) and fit["kl"] == again["kl"]      # the same seed
    assert not np.array_equal(_bits(Y), _bits(recs.map_rows(Wh, 20.0, iters=60, exag_iters=20, seed=5)["Y"].cpu().numpy()))
    rows = aff["rows"].cpu().numpy()
    assert np.isnan(Y[ZERO_ROW]).all() and np.isfinite(Y[rows]).all() and Y.shape == (N_ROWS, 2)
    assert fit["info"] == 0 and fit["lr"] == 50.0 and np.abs(Y[rows].astype(np.float64).mean(axis=0)).max() < 1e-5
    # the restatement from the same Y0 on the same CSR, centred: the fit's bits before the centring's one fp32 rounding
    Y0 = (1e-4 * np.random.default_rng(4).standard_normal((N_ROWS, 2))).astype(F32)[rows]
    csr = [aff[k].cpu().numpy() for k in ("offsets", "idx", "val")]
    wY = R.fit(Y0, *csr, 60, exag_iters=20, lr=50.0)[0].astype(np.float64)
    assert np.abs(Y[rows] - (wY - wY.mean(axis=0))).max() <= 2.0 ** -23 * np.abs(wY).max()
    P = R.dense_P(*csr, len(rows))
    assert abs(fit["kl"] - R.kl_fp64(wY, P)) < 1e-9 * max(1.0, fit["kl"])
    # placed rows: a copy of a fitted row has that row (cosine 1) as its nearest and lands inside its neighbourhood
    raw = np.random.default_rng(8).normal(size=(40, 64)).astype(F32)
    raw[7] = 0
    raw[3] = Wh_host[100] * 5
    placed = recs.map_place(fit, raw).cpu().numpy()
    assert placed.shape == (40, 2) and np.isnan(placed[7]).all() and np.isfinite(np.delete(placed, 7, 0)).all()
    Ru = ops.rownorm(_cuda(raw))
    ok = np.delete(np.arange(40), 7)
    stacked = torch.cat([Wh[aff["rows"]], Ru[_cuda(ok)]]).contiguous()
    keep = torch.zeros(len(stacked), dtype=torch.uint8, device="cuda")
    keep[:len(rows)] = 1
    nbr, cos = ops.cosine_topk(stacked, np.arange(len(rows), len(stacked)), aff["neighbours"], keep=keep)
    assert int(nbr.max()) < len(rows) and int(nbr[3, 0]) == int(np.flatnonzero(rows == 100)[0])
    p, _ = R.conditional_p(2.0 - 2.0 * cos.cpu().numpy().astype(np.float64), 20.0)
    want = (p[:, :, None] * Y[rows].astype(np.float64)[nbr.cpu().numpy()]).sum(axis=1)
    assert np.abs(placed[ok] - want).max() <= 1e-5 * np.abs(Y[rows]).max()
    lo, hi = Y[rows][nbr.cpu().numpy()[3]].min(axis=0), Y[rows][nbr.cpu().numpy()[3]].max(axis=0)
    assert (placed[3] >= lo).all() and (placed[3] <= hi).all()
    with pytest.raises(ValueError, match="width 32 on a map of width 64"):
        recs.map_place(fit, np.ones((2, 32), F32))


def _flags(**extra):
    return dict(main_df="user_stats.parquet:latest", main_df_type="parquet", project_name="anime_recommendations",
                anime_df="all_anime.csv:latest", anime_df_type="raw_data", model="wandb_anime_nn.h5:latest", model_type="h5",
                map_fn="map.csv", map_type="csv", save_map=True, **extra)


@pytest.mark.parametrize("table", ("anime", "user"))
def test_embedding_map_component(pipeline, table):  # noqa: F811
    import os
    from anime_recommendations_amd import artifacts, components as C, ops, recs, weights_io
    work, env = pipeline["work"], pipeline["env"]
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    m = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest"))
    anime_df = C.load_anime_df(pipeline["paths"]["all_anime"])
    user_ids, anime_ids = C.index_tables(m, df)
    ids, rows = (anime_ids, m["A"]) if table == "anime" else (user_ids, m["U"])
    query = str(anime_df["Name"].iloc[17]) if table == "anime" else str(int(user_ids[5]))
    query_row = C.cluster_query_row(table, query, user_ids, anime_ids, anime_df)
    max_rows = 0 if table == "anime" else 200       # the user table (300 rows) is sampled
    _run("embedding_map", _flags(map_table=table, map_perplexity=10, map_iters=120, map_seed=2, map_max_rows=max_rows,
                                 map_clusters=4, map_query=query), str(work), env)
    frame = pd.read_csv(work / (table + "_map.csv"))
    take = C.map_sample(len(ids), max_rows, 2, always=query_row)
    assert len(take) == (len(ids) if max_rows == 0 else 200) and query_row in take
    assert frame.columns.tolist() == [table + "_id"] + (["name"] if table == "anime" else []) + ["x", "y", "cluster"]
    assert frame[table + "_id"].tolist() == np.asarray(ids)[take].tolist()
    sub = np.ascontiguousarray(np.asarray(rows, np.float32)[take])
    usable = R.usable(ops.rownorm(_cuda(sub)).cpu().numpy())
    assert np.array_equal(np.isfinite(frame["x"].to_numpy()), usable) and usable.sum() > 100
    assert np.array_equal(frame["cluster"].to_numpy() >= 0, usable) and frame["cluster"].max() <= 3
    # the same seed gives the same picture: the component's CSV against the call made here
    fit = recs.map_rows(sub, perplexity=10.0, iters=120, exag_iters=30, seed=2, normalised=False)
    mine = fit["Y"].cpu().numpy()
    assert np.array_equal(_bits(frame[["x", "y"]].to_numpy(np.float32)[usable]), _bits(mine[usable]))
    meta = artifacts.artifact_metadata(table + "_map.csv:latest")
    assert meta["Filename"] == table + "_map.csv" and meta["map_table"] == table and meta["rows_mapped"] == len(take)
    assert meta["map_query"] == query and abs(meta["kl_divergence"] - fit["kl"]) < 1e-9 and meta["map_iters"] == 120
    at = int(np.searchsorted(take, query_row))
    assert np.allclose(meta["query_position"], mine[at]) and len(meta["query_neighbours"]) == 10
    near = C.map_neighbours_on_map(frame, at, 10)   # (from the CSV's decimals: the distances agree to fp32's digits)
    assert [t[0] for t in meta["query_neighbours"]] == [t[0] for t in near]
    assert np.allclose([t[2] for t in meta["query_neighbours"]], [t[2] for t in near], rtol=1e-5)
    png = work / (table + "_map.png")
    try:
        import matplotlib  # noqa: F401
        assert os.path.getsize(png) > 1000
    except ImportError:
        assert not os.path.exists(png) and "matplotlib is not importable" in open(work / "embedding_map.log").read()
