"""GPU tests of the clustered tables (anirec_kmeans_assign / anirec_kmeans_fit, ops.kmeans_assign / kmeans_fit,
recs.cluster_rows / assign_clusters, components.clusters_frame, the clusters component).

Yardstick: the NumPy restatement (tests/kmeans_restatement.py) fed with the similarities the existing
``ops.cosine_scores`` returns for the table stacked over the centroids — that kernel is not under test here, and the
header defines sim(i, c) as its chain, bit for bit.  Every comparison of C, assign, sim, count and info is exact, on
bits, NaNs included.

Shapes: test_mmr_gpu's 777-row tables (widths 32, 64, 128, 256, with the bit-identical rows 5 and 9 and the zero row 11);
K 1, 2, 7, 64 and T - 1, T, T + 1 around the tile T = anirec_kmeans_tile(width) the assign kernel stages per pass.

The twins as inits: the second twin's cluster is empty in ITERATION 1 (every tie goes to the first), so after
max_iter = 1 its centroid still has the init's bits — asserted.  From iteration 2 on it is the one centroid with cosine
1.0 to rows 5 and 9 (the first twin's centroid has moved to the mean of a few hundred rows), so they move to it and it is
updated like any other: at widths 32 .. 256 the restatement gives it 178, 181, 161 and 139 rows in the pass after the
first update.  "Empty for any number of iterations" does not hold for Lloyd's algorithm on this table; what holds, and is
asserted at every max_iter, is that the kernels equal the restatement, whose update keeps the bits of every cluster
that is empty in that iteration.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest

import kmeans_restatement as K
import poison
from test_components_gpu import _run, pipeline  # noqa: F401  (the components' pipeline fixture, as it is)
from test_mmr_gpu import N_ROWS, TWIN_A, TWIN_B, WIDTHS, ZERO_ROW, _bits, _cuda, _table

pytestmark = pytest.mark.gpu
NAN_BITS = np.uint32(0x7FC00000)
KS_ASSIGN = (1, 2, 7, 64, "T-1", "T", "T+1")
FIT_CASES = [(dim, k) for dim in WIDTHS for k in (2, 7, 64)] + [(128, "T+1"), (256, "T+1")]
MAX_ITERS = (1, 2, 5, 40)


def _k(dim, k):
    from anime_recommendations_amd import _lib
    T = _lib.kmeans_tile(dim)
    return {"T-1": T - 1, "T": T, "T+1": T + 1}.get(k, k)


def _sims_fn(Wh):
    """C -> the [n, k] fp32 similarities of the device table ``Wh`` against the centroids ``C``: column c is
    ``ops.cosine_scores`` of the stacked table at row n + c"""
    import torch
    from anime_recommendations_amd import ops
    n = int(Wh.shape[0])

    def sims(C):
        stacked = torch.cat([Wh, _cuda(np.ascontiguousarray(C, np.float32))])
        return torch.stack([ops.cosine_scores(stacked, n + c)[:n] for c in range(len(C))], dim=1).cpu().numpy()
    return sims


def _same_fit(got, ref, what):
    C, a, s, count, iters, converged = got
    rC, ra, rs, rcount, rinfo = ref
    assert (int(iters), int(bool(converged))) == tuple(rinfo), (what, iters, converged, rinfo)
    assert np.array_equal(a.cpu().numpy(), ra), what
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(rs)), what
    assert np.array_equal(count.cpu().numpy(), rcount), what
    assert np.array_equal(_bits(C.cpu().numpy()), _bits(rC)), what


# ---- assign -----------------------------------------------------------------------------------------------------
def _centroids(dim, k):
    """k random unit vectors; from k = 7 on centroid 3 is NaN and centroid 5 a bit-copy of centroid 2; at k = 2 the
    second is a bit-copy of the first"""
    rng = np.random.default_rng(5000 + 10 * dim + k)
    C = rng.normal(size=(k, dim))
    C = (C / np.linalg.norm(C, axis=1, keepdims=True)).astype(np.float32)
    if k >= 7:
        C[3] = np.nan
        C[5] = C[2]
    elif k == 2:
        C[1] = C[0]
    return C


_ASSIGN_REFS = {}


def _assign_ref(dim, k):
    if (dim, k) not in _ASSIGN_REFS:
        Wh, Wh_host, _ = _table(dim)
        C = _centroids(dim, k)
        _ASSIGN_REFS[(dim, k)] = (C,) + K.assign(_sims_fn(Wh)(C), K.usable(Wh_host))
    return _ASSIGN_REFS[(dim, k)]


@pytest.mark.parametrize("k", KS_ASSIGN)
@pytest.mark.parametrize("dim", WIDTHS)
def test_assign_equals_the_restatement(dim, k):
    from anime_recommendations_amd import ops
    k = _k(dim, k)
    Wh = _table(dim)[0]
    C, ra, rs = _assign_ref(dim, k)
    a, s = ops.kmeans_assign(Wh, _cuda(C))
    a, s = a.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(a, ra) and np.array_equal(_bits(s), _bits(rs))
    # the planted content did what it is there for (checked on the reference, which the kernel has just equalled)
    assert ra[ZERO_ROW] == -1 and _bits(rs[ZERO_ROW]) == NAN_BITS
    assert (np.delete(ra, ZERO_ROW) >= 0).all() and ra[TWIN_A] == ra[TWIN_B] and _bits(rs[TWIN_A]) == _bits(rs[TWIN_B])
    if k >= 7:
        assert (ra != 3).all() and (ra != 5).all()              # the NaN centroid, the second of two identical ones
        if k == 7:
            assert (ra == 2).any()                              # ... whose first copy is picked
    elif k == 2:
        assert (np.delete(ra, ZERO_ROW) == 0).all()
    if k > 64:
        assert len(np.unique(ra)) > 64                          # picks from every part of a long centroid list


@pytest.mark.parametrize("dim", WIDTHS)
def test_a_subset_of_the_rows_gives_the_same_bits(dim):
    """a row's pick depends on that row and C alone: 301 rows in another order, the zero row among them, as a call of
    their own — another grid, other lanes"""
    from anime_recommendations_amd import ops
    Wh = _table(dim)[0]
    rows = np.random.default_rng(dim).permutation(N_ROWS)[:300]
    rows = np.concatenate([rows[rows != ZERO_ROW], [ZERO_ROW]])
    for k in (7, _k(dim, "T+1")):
        C, ra, rs = _assign_ref(dim, k)
        a, s = ops.kmeans_assign(Wh[_cuda(rows)].contiguous(), _cuda(C))
        assert np.array_equal(a.cpu().numpy(), ra[rows]) and np.array_equal(_bits(s.cpu().numpy()), _bits(rs[rows]))
        assert a[-1].item() == -1


# ---- fit --------------------------------------------------------------------------------------------------------
def _init_rows(dim, k):
    """the rows whose unit rows are the first centroids: from k = 7 on the twins 5 and 9 and the zero row 11 (a NaN
    centroid) lead them"""
    rng = np.random.default_rng(dim * 31 + k)
    pool = np.setdiff1d(np.arange(N_ROWS), [TWIN_A, TWIN_B, ZERO_ROW])
    if k >= 7:
        return np.concatenate([[TWIN_A, TWIN_B, ZERO_ROW], rng.choice(pool, k - 3, replace=False)])
    return rng.choice(pool, k, replace=False)


_FIT_REFS = {}


def _fit_ref(dim, rows, max_iter):
    key = (dim, tuple(int(r) for r in rows), max_iter)
    if key not in _FIT_REFS:
        Wh, Wh_host, _ = _table(dim)
        _FIT_REFS[key] = K.fit(Wh_host, Wh_host[np.asarray(rows)], max_iter, _sims_fn(Wh))
    return _FIT_REFS[key]


@pytest.mark.parametrize("max_iter", MAX_ITERS)
@pytest.mark.parametrize("dim,k", FIT_CASES)
def test_fit_equals_the_restatement(dim, k, max_iter):
    from anime_recommendations_amd import ops
    k = _k(dim, k)
    Wh, Wh_host, _ = _table(dim)
    rows = _init_rows(dim, k)
    ref = _fit_ref(dim, rows, max_iter)
    print("width %d, k %d, max_iter %d: the restatement ran %d iterations, converged %d" % ((dim, k, max_iter) + tuple(ref[4])))
    if max_iter == 40:
        assert ref[4][1] == 1 and ref[4][0] < 40                # the restatement itself stops early: the device flag runs
    C0 = Wh[_cuda(rows)]
    before = C0.clone()
    _same_fit(ops.kmeans_fit(Wh, C0, max_iter), ref, (dim, k, max_iter))
    assert np.array_equal(_bits(C0.cpu().numpy()), _bits(before.cpu().numpy()))      # the caller's C0 is not modified
    rC, ra, rs, rcount, _ = ref
    assert ra[ZERO_ROW] == -1 and rcount.sum() == N_ROWS - 1 and np.array_equal(rcount, np.bincount(ra[ra >= 0], minlength=k))
    if k >= 7:
        assert np.isnan(rC[2]).all() and rcount[2] == 0        # the zero row as an init: a NaN centroid, never picked
        if max_iter == 1:                                       # the second twin: empty in iteration 1, its bits kept
            assert np.array_equal(_bits(rC[1]), _bits(Wh_host[TWIN_B]))
            assert not np.array_equal(_bits(rC[0]), _bits(Wh_host[TWIN_A]))


@pytest.mark.parametrize("dim", WIDTHS)
def test_the_twins_and_the_zero_row_as_the_only_inits(dim):
    from anime_recommendations_amd import ops
    Wh, Wh_host, _ = _table(dim)
    rows = np.array([TWIN_A, TWIN_B, ZERO_ROW])
    a1, _ = K.assign(_sims_fn(Wh)(Wh_host[rows]), K.usable(Wh_host))
    assert (np.delete(a1, ZERO_ROW) == 0).all()                 # iteration 1: every row ties, the first twin takes all
    for max_iter in (1, 2, 5, 40):
        ref = _fit_ref(dim, rows, max_iter)
        C, a, s, count, iters, converged = got = ops.kmeans_fit(Wh, Wh[_cuda(rows)], max_iter)
        _same_fit(got, ref, (dim, max_iter))
        assert np.isnan(C[2].cpu().numpy()).all() and int(count[2]) == 0 and int((a == 2).sum()) == 0
        if max_iter == 1:
            assert np.array_equal(_bits(C[1].cpu().numpy()), _bits(Wh_host[TWIN_B]))
    assert ref[4][1] == 1


# ---- order-free -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,k", [(32, 7), (64, 64), (128, 64), (128, "T+1"), (256, 7), (256, 64)])
def test_permuted_rows_give_the_same_centroids(dim, k):
    """the sums are integers: the rows in another order — other lanes, other workgroups, another arrival order of the
    atomics — give bit-identical centroids and the permuted assignments (both forms of the sums kernel: partials in LDS
    at k * width * 8 <= 64 KiB, global atomics beyond)"""
    from anime_recommendations_amd import ops
    k = _k(dim, k)
    Wh = _table(dim)[0]
    C0 = Wh[_cuda(_init_rows(dim, k))]
    C, a, s, count, iters, converged = ops.kmeans_fit(Wh, C0, 5)
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(N_ROWS)
        Cp, ap, sp, countp, itersp, convergedp = ops.kmeans_fit(Wh[_cuda(perm)].contiguous(), C0, 5)
        assert np.array_equal(_bits(Cp.cpu().numpy()), _bits(C.cpu().numpy()))
        assert np.array_equal(ap.cpu().numpy(), a.cpu().numpy()[perm])
        assert np.array_equal(_bits(sp.cpu().numpy()), _bits(s.cpu().numpy()[perm]))
        assert np.array_equal(countp.cpu().numpy(), count.cpu().numpy()) and (itersp, convergedp) == (iters, converged)
    C2 = ops.kmeans_fit(Wh, C0, 5)[0]                           # and twice the same call
    assert np.array_equal(_bits(C2.cpu().numpy()), _bits(C.cpu().numpy()))


# ---- workspace --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", poison.ORDER)
def test_a_dirty_workspace_and_dirty_outputs_change_nothing(byte):
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    for dim, k, max_iter in ((32, 7, 5), (128, "T+1", 2), (256, 64, 40)):
        k = _k(dim, k)
        Wh = _table(dim)[0]
        rows = _init_rows(dim, k)
        log = []
        with poison.poisoned(byte, log):
            got = ops.kmeans_fit(Wh, Wh[_cuda(rows)], max_iter)
        # assign, sim, count, info and the workspace
        assert sorted(log) == sorted([N_ROWS * 4, N_ROWS * 4, k * 4, 8, lib.anirec_kmeans_workspace_bytes(N_ROWS, k, dim)])
        _same_fit(got, _fit_ref(dim, rows, max_iter), (byte, dim))
    log = []
    with poison.poisoned(byte, log):
        a, s = ops.kmeans_assign(_table(64)[0], _cuda(_centroids(64, 7)))
    assert log == [N_ROWS * 4, N_ROWS * 4]
    assert np.array_equal(a.cpu().numpy(), _assign_ref(64, 7)[1]) and np.array_equal(_bits(s.cpu().numpy()), _bits(_assign_ref(64, 7)[2]))


def _raw_fit(dim, C0, max_iter, n_rows=N_ROWS, k=None, ws_short=0, null=None, fill=0x3F, dim_arg=None):
    """anirec_kmeans_fit itself, outputs and workspace pre-filled with ``fill`` bytes.  Returns (status, tensors)."""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    kk = C0.shape[0]
    t = dict(What=_table(dim)[0], C=C0.clone(), assign=torch.empty(N_ROWS, dtype=torch.int32, device="cuda"),
             sim=torch.empty(N_ROWS, dtype=torch.float32, device="cuda"), count=torch.empty(kk, dtype=torch.int32, device="cuda"),
             info=torch.empty(2, dtype=torch.int32, device="cuda"),
             ws=torch.empty(int(lib.anirec_kmeans_workspace_bytes(N_ROWS, kk, dim)), dtype=torch.uint8, device="cuda"))
    for n in ("assign", "sim", "count", "info", "ws"):
        poison.fill(t[n], fill)
    p = {n: (None if n == null else _lib.ptr(v)) for n, v in t.items()}
    st = lib.anirec_kmeans_fit(p["What"], dim if dim_arg is None else dim_arg, n_rows, p["C"], kk if k is None else k, max_iter,
                               p["assign"], p["sim"], p["count"], p["info"], p["ws"], t["ws"].numel() - ws_short,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, t


def test_einval_returns_before_writing():
    import torch
    dim, k = 128, 7
    C0 = _table(dim)[0][_cuda(_init_rows(dim, k))]
    cases = [dict(dim_arg=48), dict(dim_arg=0), dict(dim_arg=512), dict(n_rows=0), dict(n_rows=-5), dict(k=0), dict(k=-1),
             dict(k=4097), dict(max_iter=0), dict(max_iter=1001), dict(ws_short=1), dict(k=8)]
    cases += [dict(null=n) for n in ("What", "C", "assign", "sim", "count", "info", "ws")]
    for kw in cases:
        kw = dict(kw)
        st, t = _raw_fit(dim, C0, kw.pop("max_iter", 5), **kw)
        assert st == -1, kw
        assert all(bool((t[n].view(-1).view(torch.uint8) == 0x3F).all()) for n in ("assign", "sim", "count", "info", "ws")), kw
        assert np.array_equal(_bits(t["C"].cpu().numpy()), _bits(C0.cpu().numpy())), kw
    st, t = _raw_fit(dim, C0, 5)                                # and the same call, untampered, runs
    assert st == 0
    _same_fit((t["C"], t["assign"], t["sim"], t["count"]) + tuple(t["info"].tolist()), _fit_ref(dim, _init_rows(dim, k), 5), "raw")


def test_the_fit_is_graph_capturable():
    """captured into a graph the call runs nothing; every replay writes the restatement's bits, the second one from
    the workspace and the outputs the first one left"""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    for dim, k, max_iter in ((128, 7, 40), (256, "T+1", 2)):
        k = _k(dim, k)
        Wh = _table(dim)[0]
        rows = _init_rows(dim, k)
        C0 = Wh[_cuda(rows)].clone()
        C = C0.clone()
        outs = [poison.fill(torch.empty(n, dtype=dt, device="cuda"), 0x3F)
                for n, dt in ((N_ROWS, torch.int32), (N_ROWS, torch.float32), (k, torch.int32), (2, torch.int32))]
        ws = poison.fill(torch.empty(int(lib.anirec_kmeans_workspace_bytes(N_ROWS, k, dim)), dtype=torch.uint8, device="cuda"), 0x3F)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            st = lib.anirec_kmeans_fit(_lib.ptr(Wh), dim, N_ROWS, _lib.ptr(C), k, max_iter, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                       _lib.ptr(outs[2]), _lib.ptr(outs[3]), _lib.ptr(ws), ws.numel(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        torch.cuda.synchronize()
        assert all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in outs + [ws])      # captured, not run
        for _ in range(2):
            C.copy_(C0)
            graph.replay()
            torch.cuda.synchronize()
            _same_fit((C, outs[0], outs[1], outs[2]) + tuple(outs[3].tolist()), _fit_ref(dim, rows, max_iter), "graph replay")


# ---- planted clusters -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (32, 128, 256))
def test_planted_clusters_are_recovered(dim):
    """777 rows around 6 random unit directions, noise of length about 0.3 (N(0, 0.3^2 / width) a coordinate), row i in
    cluster i % 6, the first centroids one member of each (rows 0 .. 5).  The labels come back exactly and the fit
    stops in iteration 2.  Both follow from two margins asserted on the input in float64: every row is nearer its own
    cluster's init row than any other init row, and nearer its own cluster's mean direction than any other's, each
    by more than 1e-3 — against a cosine error below 256 * 2**-24 < 2e-5 for the fp32 chains of unit rows (rownorm's
    rounding and the centroids' fp32 rounding, 2**-24 relative each, and q's 2**-31 included)."""
    from anime_recommendations_amd import ops, recs
    rng = np.random.default_rng(7 + dim)
    centres = rng.normal(size=(6, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    label = np.arange(N_ROWS) % 6
    W = (centres[label] + 0.3 * rng.normal(size=(N_ROWS, dim)) / np.sqrt(dim)).astype(np.float32)
    Wn = W.astype(np.float64) / np.linalg.norm(W.astype(np.float64), axis=1, keepdims=True)
    own = np.zeros((N_ROWS, 6), bool)
    own[np.arange(N_ROWS), label] = True
    means = np.stack([Wn[label == c].sum(axis=0) for c in range(6)])
    means /= np.linalg.norm(means, axis=1, keepdims=True)
    for cents, what in ((Wn[:6], "init rows"), (means, "mean directions")):
        cos = Wn @ cents.T
        margin = (cos[own] - np.where(own, -np.inf, cos).max(axis=1)).min()
        print("width %d, %s: smallest margin %.4f" % (dim, what, margin))
        assert margin > 1e-3
    Wh = ops.rownorm(_cuda(W))
    out = recs.cluster_rows(Wh, 6, init=np.arange(6), max_iter=50)
    assert np.array_equal(out["assign"].cpu().numpy(), label) and (out["iters"], out["converged"]) == (2, True)
    assert out["count"].cpu().numpy().tolist() == np.bincount(label).tolist() and float(out["sim"].min()) > 0.85
    assert np.array_equal(out["init_rows"], np.arange(6))
    got = ops.kmeans_fit(Wh, Wh[:6], 50)
    _same_fit(got, K.fit(Wh.cpu().numpy(), Wh[:6].cpu().numpy(), 50, _sims_fn(Wh)), dim)


# ---- host layers ------------------------------------------------------------------------------------------------
def test_cluster_rows_and_assign_clusters():
    import torch
    from anime_recommendations_amd import ops, recs
    dim, k = 64, 7
    Wh, Wh_host, _ = _table(dim)
    fit = recs.cluster_rows(Wh[:600], k, seed=3, max_iter=30)
    usable = np.flatnonzero(K.usable(Wh_host[:600]))
    rows = np.random.default_rng(3).choice(usable, size=k, replace=False)
    assert np.array_equal(fit["init_rows"], rows) and ZERO_ROW not in rows and len(set(rows.tolist())) == k
    _same_fit(ops.kmeans_fit(Wh[:600], Wh[_cuda(rows)], 30), (fit["C"].cpu().numpy(), fit["assign"].cpu().numpy(),
              fit["sim"].cpu().numpy(), fit["count"].cpu().numpy(), (fit["iters"], int(fit["converged"]))), "cluster_rows")
    again = recs.cluster_rows(Wh[:600], k, seed=3, max_iter=30)
    assert np.array_equal(_bits(again["C"].cpu().numpy()), _bits(fit["C"].cpu().numpy()))
    assert not np.array_equal(recs.cluster_rows(Wh[:600], k, seed=4, max_iter=30)["init_rows"], rows)
    # rows outside the fitted table: the same call as ops.kmeans_assign, no refit
    a, s = recs.assign_clusters(fit["C"], Wh[600:])
    ra, rs = ops.kmeans_assign(Wh[600:].contiguous(), fit["C"])
    assert np.array_equal(a.cpu().numpy(), ra.cpu().numpy()) and np.array_equal(_bits(s.cpu().numpy()), _bits(rs.cpu().numpy()))
    ka, ks = K.assign(_sims_fn(Wh[600:].contiguous())(fit["C"].cpu().numpy()), K.usable(Wh_host[600:]))
    assert np.array_equal(a.cpu().numpy(), ka) and np.array_equal(_bits(s.cpu().numpy()), _bits(ks))
    # a host array is a raw table, normalised here
    raw = np.random.default_rng(9).normal(size=(50, dim)).astype(np.float32) * 3
    a2, s2 = recs.assign_clusters(fit["C"].cpu().numpy(), raw)
    a3, s3 = ops.kmeans_assign(ops.rownorm(_cuda(raw)), fit["C"])
    assert np.array_equal(a2.cpu().numpy(), a3.cpu().numpy()) and np.array_equal(_bits(s2.cpu().numpy()), _bits(s3.cpu().numpy()))
    with pytest.raises(ValueError, match="only 2 usable rows"):
        recs.cluster_rows(torch.cat([Wh[:2], Wh[ZERO_ROW:ZERO_ROW + 1]]), 3)


def _flags(**extra):
    return dict(main_df="user_stats.parquet:latest", main_df_type="parquet", project_name="anime_recommendations",
                anime_df="all_anime.csv:latest", anime_df_type="raw_data", model="wandb_anime_nn.h5:latest", model_type="h5",
                clusters_fn="clusters.csv", clusters_type="csv", save_clusters=True, **extra)


@pytest.mark.parametrize("table", ("anime", "user"))
def test_clusters_component(pipeline, table):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, ops, weights_io
    work, env = pipeline["work"], pipeline["env"]
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    m = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest"))
    anime_df = C.load_anime_df(pipeline["paths"]["all_anime"])
    user_ids, anime_ids = C.index_tables(m, df)
    ids, rows = (anime_ids, m["A"]) if table == "anime" else (user_ids, m["U"])
    query = str(anime_df["Name"].iloc[17]) if table == "anime" else str(int(user_ids[5]))
    query_row = C.cluster_query_row(table, query, user_ids, anime_ids, anime_df)
    _run("clusters", _flags(cluster_table=table, n_clusters=8, cluster_iters=30, cluster_seed=1, cluster_top=4,
                            cluster_query=query), str(work), env)
    frame = pd.read_csv(work / (table + "_clusters.csv"))
    assignments = pd.read_csv(work / (table + "_assignments_clusters.csv"))
    assert frame.columns.tolist() == C.CLUSTERS_COLUMNS and frame["cluster"].tolist() == list(range(8))
    assert assignments.columns.tolist() == [table + "_id", "cluster", "similarity"]
    assert assignments[table + "_id"].tolist() == np.asarray(ids).tolist()
    usable = K.usable(ops.rownorm(_cuda(np.asarray(rows, np.float32))).cpu().numpy())
    assert frame["size"].sum() == usable.sum() and usable.sum() > 8
    assert np.array_equal(assignments["cluster"].to_numpy() >= 0, usable)
    assert frame["size"].tolist() == np.bincount(assignments["cluster"][assignments["cluster"] >= 0], minlength=8).tolist()
    for c in range(8):
        members = assignments[assignments["cluster"] == c]
        if len(members):
            assert abs(frame["mean_similarity"][c] - members["similarity"].mean()) < 1e-6
            shown = frame["top_members"][c].split(" | ")
            assert len(shown) == min(4, len(members))
            if table == "user":
                best = members.sort_values(["similarity"], ascending=False, kind="stable")[table + "_id"].tolist()[:len(shown)]
                assert [int(x) for x in shown] == best or members["similarity"].duplicated().any()
    assert frame["top_genres"].notna().any()
    for name in (table + "_clusters.csv", table + "_assignments_clusters.csv"):
        meta = artifacts.artifact_metadata(name + ":latest")
        assert meta["Filename"] == name and meta["cluster_table"] == table and meta["n_clusters"] == 8
        assert meta["cluster_query"] == query and meta["query_cluster"] == int(assignments["cluster"].iloc[query_row])
        assert 0 <= meta["query_cluster"] < 8 and 1 <= meta["iterations"] <= 30 and meta["cluster_seed"] == 1
