"""CPU tests of the clustered tables: the restatement's own rules on hand-built cases, the binding and the entry points'
refusals (no device needed), the ops / recs checks and the clusters component's flag surface."""
import ctypes
import os

import numpy as np
import pytest

import kmeans_restatement as K
from component_cli import load_component

from anime_recommendations_amd import _lib, build, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = np.uint32(0x7FC00000)
INF = np.float32(np.inf)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _unit(rows):
    W = np.asarray(rows, np.float64)
    return (W / np.linalg.norm(W, axis=1, keepdims=True)).astype(np.float32)


def _dot_sims(What):
    """a sims callback for ``K.fit`` from a plain float32 matmul: the hand-built cases do not hang on the chain's bits"""
    with np.errstate(invalid="ignore"):
        return lambda C: (What.astype(np.float32) @ np.asarray(C, np.float32).T).astype(np.float32)


# ---- the restatement on hand-built cases ------------------------------------------------------------------------
def test_a_tie_goes_to_the_lowest_centroid():
    S = np.array([[0.5, 0.75, 0.75, 0.1], [0.25, 0.25, 0.25, 0.25], [0.1, 0.2, 0.3, 0.3]], np.float32)
    a, s = K.assign(S, [True] * 3)
    assert a.tolist() == [1, 0, 2] and s.tolist() == [0.75, 0.25, np.float32(0.3)]


def test_negative_zero_ties_with_positive_zero():
    S = np.array([[-0.0, 0.0, -0.5], [0.0, -0.0, 0.0], [-1.0, -0.0, 0.0]], np.float32)
    a, s = K.assign(S, [True] * 3)
    assert a.tolist() == [0, 0, 1]
    assert np.signbit(s).tolist() == [True, False, True]       # the first of the tied zeros, with its own sign


def test_a_nan_sim_is_never_picked_and_inf_is_a_number():
    S = np.array([[np.nan, 0.25, np.nan, 0.5], [np.nan, -INF, np.nan, np.nan], [np.nan, np.nan, np.nan, np.nan],
                  [0.5, INF, INF, np.nan], [-INF, -INF, -1.0, np.nan]], np.float32)
    a, s = K.assign(S, [True] * 5)
    assert a.tolist() == [3, 1, -1, 1, 2]
    assert s[0] == 0.5 and s[1] == -INF and _bits(s[2]) == NAN_BITS and s[3] == INF and s[4] == -1.0


def test_an_unusable_row_gets_minus_one():
    What = np.array([[1, 0], [np.nan, 0], [0, np.inf], [2, -2], [0, 2.0000002], [0, 0]], np.float32)
    ok = K.usable(What)
    assert ok.tolist() == [True, False, False, True, False, True]
    S = np.full((6, 3), 0.5, np.float32)
    a, s = K.assign(S, ok)
    assert a.tolist() == [0, -1, -1, 0, -1, 0]
    assert (_bits(s[[1, 2, 4]]) == NAN_BITS).all() and (s[[0, 3, 5]] == 0.5).all()


def test_q_rounds_to_the_nearest_even_integer():
    x = np.array([1.0, -1.0, 2.0, 2.0 ** -31, 3 * 2.0 ** -31, -(2.0 ** -31), 2.0 ** -32, 0.1], np.float32)
    q = K.quantise(x)
    assert q.dtype == np.int64
    assert q[:7].tolist() == [2 ** 30, -2 ** 30, 2 ** 31, 0, 2, 0, 0]       # halves go to the even neighbour
    assert q[7] == int(np.rint(float(np.float32(0.1)) * 2 ** 30))


def test_update_sums_integers_and_normalises_in_fp64():
    What = _unit([[3, 4], [4, 3], [-1, 0], [0, 1]])
    C = np.array([[1, 0], [0, 1], [0.6, 0.8]], np.float32)
    a = np.array([0, 0, 1, -1], np.int32)
    C2, count = K.update(What, a, C)
    assert count.tolist() == [2, 1, 0]
    S0 = [int(K.quantise(What[0])[t]) + int(K.quantise(What[1])[t]) for t in range(2)]      # Python ints
    d = [float(v) for v in S0]
    nn = 0.0
    for t in range(2):
        nn = nn + d[t] * d[t]
    want = np.array([d[t] / np.sqrt(nn) for t in range(2)]).astype(np.float32)
    assert np.array_equal(_bits(C2[0]), _bits(want))
    assert np.array_equal(_bits(C2[1]), _bits(np.array([-1, 0], np.float32)))
    # order-free: the same rows in another order give the same bits
    C3, _ = K.update(What[[3, 1, 2, 0]], a[[3, 1, 2, 0]], C)
    assert np.array_equal(_bits(C3), _bits(C2))


def test_an_empty_cluster_and_a_zero_sum_keep_their_bits():
    What = _unit([[1, 0], [-1, 0], [0, 1]])
    C = np.array([[0.123, -0.5], [0.25, 0.75], [-0.0, 7.0]], np.float32)
    C2, count = K.update(What, np.array([1, 1, 2], np.int32), C)
    assert count.tolist() == [0, 2, 1]
    assert np.array_equal(_bits(C2[0]), _bits(C[0]))                        # nothing assigned: kept
    assert np.array_equal(_bits(C2[1]), _bits(C[1]))                        # the members cancel: nn == 0, kept
    assert np.array_equal(_bits(C2[2]), _bits(np.array([0, 1], np.float32)))


def test_a_nan_centroid_stays_nan():
    What = _unit([[1, 0], [0.9, 0.1], [0, 1], [0.1, 0.9]])
    C0 = np.stack([What[0], np.array([np.nan, np.nan], np.float32), What[2]])
    C0[1].view(np.uint32)[:] = 0x7FC01234                                   # a NaN with a payload: its bits are kept
    C, a, s, count, info = K.fit(What, C0, 10, _dot_sims(What))
    assert a.tolist() == [0, 0, 2, 2] and count.tolist() == [2, 0, 2] and info == (2, 1)
    assert (_bits(C[1]) == np.uint32(0x7FC01234)).all()


def test_the_stop_at_changed_zero_leaves_c_untouched():
    What = _unit([[1, 0.1], [1, -0.1], [0.1, 1], [-0.1, 1]])
    seen = []

    def sims(C):
        seen.append(np.array(C, copy=True))
        return _dot_sims(What)(C)

    C, a, s, count, info = K.fit(What, What[[0, 2]], 20, sims)
    assert info == (2, 1) and len(seen) == 2 and a.tolist() == [0, 0, 1, 1] and count.tolist() == [2, 2]
    assert np.array_equal(_bits(C), _bits(seen[-1]))                        # the C of the last assign pass is returned
    a1, s1 = K.assign(sims(C), K.usable(What))
    assert np.array_equal(a1, a) and np.array_equal(_bits(s1), _bits(s))    # and the outputs belong to it
    assert not np.array_equal(_bits(C), _bits(What[[0, 2]]))                # (iteration 1 did move it)


def test_a_run_that_does_not_converge_ends_with_a_final_pass():
    rng = np.random.default_rng(3)
    What = _unit(rng.normal(size=(200, 4)))
    C0 = What[:7]
    full = K.fit(What, C0, 40, _dot_sims(What))
    assert full[4][1] == 1 and full[4][0] > 3
    seen = []

    def sims(C):
        seen.append(np.array(C, copy=True))
        return _dot_sims(What)(C)

    C, a, s, count, info = K.fit(What, C0, 2, sims)
    assert info == (2, 0) and len(seen) == 3                                # two iterations and the final pass
    assert np.array_equal(_bits(C), _bits(seen[2]))
    a2, s2 = K.assign(_dot_sims(What)(C), K.usable(What))
    assert np.array_equal(a, a2) and np.array_equal(_bits(s), _bits(s2)) and count.sum() == 200
    assert np.array_equal(count, np.bincount(a, minlength=7))


# ---- the binding, the tile query and the entry points' refusals -------------------------------------------------
def test_symbols_declared_bound_and_exported():
    P = _lib.PROTOTYPES
    assert len(P["anirec_kmeans_tile"][1]) == 1 and P["anirec_kmeans_tile"][0] is ctypes.c_size_t
    assert len(P["anirec_kmeans_assign"][1]) == 8 and P["anirec_kmeans_assign"][0] is ctypes.c_int
    assert len(P["anirec_kmeans_workspace_bytes"][1]) == 3 and P["anirec_kmeans_workspace_bytes"][0] is ctypes.c_size_t
    assert len(P["anirec_kmeans_fit"][1]) == 13 and P["anirec_kmeans_fit"][0] is ctypes.c_int
    assert _lib.ABI_VERSION == 5 and "anirec_kmeans.hip" in build.SOURCES
    assert _lib.KMEANS_MAX_K == 4096 and _lib.KMEANS_MAX_ITER == 1000
    header = open(os.path.join(ROOT, "include", "anirec.h")).read()
    for name in ("anirec_kmeans_tile", "anirec_kmeans_assign", "anirec_kmeans_workspace_bytes", "anirec_kmeans_fit"):
        assert name + "(" in header
    assert "#define ANIREC_KMEANS_MAX_K 4096" in header and "#define ANIREC_ABI_VERSION 5" in header
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.anirec_abi_version() == 5
    for dim in _lib.WIDTHS:
        t = lib.anirec_kmeans_tile(dim)
        assert t == _lib.kmeans_tile(dim) == 32768 // dim and t >= 128
        assert lib.anirec_kmeans_workspace_bytes(100, 7, dim) >= 7 * dim * 8
        assert lib.anirec_kmeans_workspace_bytes(100, 4096, dim) >= 4096 * dim * 8
        for bad in ((0, 7), (-1, 7), (100, 0), (100, 4097)):
            assert lib.anirec_kmeans_workspace_bytes(bad[0], bad[1], dim) == 0
    for dim in (0, 16, 48, 100, 512, -32):
        assert lib.anirec_kmeans_tile(dim) == 0 and lib.anirec_kmeans_workspace_bytes(100, 7, dim) == 0
        with pytest.raises(ValueError, match="embedding_size"):
            _lib.kmeans_tile(dim)


def test_entry_points_refuse_bad_arguments_without_a_device():
    build.build(verbose=False)
    lib = _lib.load()
    fake = 4096         # never followed: every refusal comes before anything is enqueued

    def assign(dim=128, n_rows=50, k=7, **null):
        p = {n: (None if null.get(n) else fake) for n in ("What", "C", "assign", "sim")}
        return lib.anirec_kmeans_assign(p["What"], dim, n_rows, p["C"], k, p["assign"], p["sim"], None)

    def fit(dim=128, n_rows=50, k=7, max_iter=5, ws_bytes=None, ws=fake, **null):
        p = {n: (None if null.get(n) else fake) for n in ("What", "C", "assign", "sim", "count", "info")}
        need = lib.anirec_kmeans_workspace_bytes(50, 7, 128) if ws_bytes is None else ws_bytes
        return lib.anirec_kmeans_fit(p["What"], dim, n_rows, p["C"], k, max_iter, p["assign"], p["sim"], p["count"],
                                     p["info"], ws, need, None)

    shape = (dict(dim=48), dict(dim=0), dict(dim=512), dict(dim=-128), dict(n_rows=0), dict(n_rows=-3), dict(k=0),
             dict(k=-1), dict(k=4097))
    for kw in shape:
        assert assign(**kw) == -1, kw
        assert fit(**kw) == -1, kw
    for kw in (dict(max_iter=0), dict(max_iter=-1), dict(max_iter=1001)):
        assert fit(**kw) == -1, kw
    for name in ("What", "C", "assign", "sim"):
        assert assign(**{name: True}) == -1, name
    for name in ("What", "C", "assign", "sim", "count", "info"):
        assert fit(**{name: True}) == -1, name
    assert fit(ws=None) == -1
    need = lib.anirec_kmeans_workspace_bytes(50, 7, 128)
    assert fit(ws_bytes=need - 1) == -1 and fit(ws_bytes=0) == -1
    assert fit(k=8) == -1                                       # a workspace sized for 7 centroids is too small for 8


# ---- the host layers --------------------------------------------------------------------------------------------
def test_ops_check_kmeans_messages():
    assert ops.check_kmeans(128, 64, 50) == (128, 64, 50) and ops.check_kmeans(32, 4096, 1000) == (32, 4096, 1000)
    assert ops.check_kmeans(256, 1) == (256, 1, 1)
    with pytest.raises(ValueError, match="embedding_size"):
        ops.check_kmeans(48, 10, 5)
    for k in (0, -1, 4097):
        with pytest.raises(ValueError, match=r"k = %d centroids must be in 1 .. 4096" % k):
            ops.check_kmeans(128, k, 5)
    for it in (0, -2, 1001):
        with pytest.raises(ValueError, match=r"max_iter = %d must be in 1 .. 1000" % it):
            ops.check_kmeans(128, 10, it)
    import torch
    What, C = torch.zeros(50, 128), torch.zeros(7, 64)
    with pytest.raises(ValueError, match="of one width"):
        ops.kmeans_assign(What, C)
    with pytest.raises(ValueError, match="of one width"):
        ops.kmeans_fit(What, C[0], 5)
    with pytest.raises(ValueError, match="no rows"):
        ops.kmeans_assign(What[:0], torch.zeros(7, 128))
    with pytest.raises(ValueError, match="max_iter = 0"):
        ops.kmeans_fit(What, torch.zeros(7, 128), 0)
    with pytest.raises(ValueError, match="k = 4097"):
        ops.kmeans_assign(What, torch.zeros(4097, 128))


def test_cluster_rows_refusals_need_no_gpu():
    W = np.random.default_rng(0).normal(size=(5, 32)).astype(np.float32)
    with pytest.raises(ValueError, match="k = 6 clusters but the table has only 5 usable rows"):
        recs.cluster_rows(W, 6)
    with pytest.raises(ValueError, match="k = 0"):
        recs.cluster_rows(W, 0)
    with pytest.raises(ValueError, match="max_iter = 1001"):
        recs.cluster_rows(W, 2, max_iter=1001)
    with pytest.raises(ValueError, match=r"init must be 3 row indices or a float \[3, 32\] array"):
        recs.cluster_rows(W, 3, init=np.zeros((3, 16), np.float32))
    with pytest.raises(ValueError, match="init must be 3 row indices"):
        recs.cluster_rows(W, 3, init=np.zeros((2, 32), np.float32))
    with pytest.raises(ValueError, match="init must be 3 row indices"):
        recs.cluster_rows(W, 3, init=[0, 1])
    with pytest.raises(ValueError, match="init row out of range"):
        recs.cluster_rows(W, 3, init=[0, 1, 5])
    with pytest.raises(ValueError, match="embedding_size"):
        recs.cluster_rows(W[:, :20], 2)
    with pytest.raises(ValueError, match=r"\[n_rows, width\]"):
        recs.cluster_rows(W[0], 2)


# ---- the component's flag surface -------------------------------------------------------------------------------
def test_clusters_parser_and_mlproject_agree():
    mod = load_component("clusters")
    from anime_recommendations_amd import components as C
    assert mod.STR_FLAGS == ["main_df", "main_df_type", "project_name", "anime_df", "anime_df_type", "model", "model_type",
                             "clusters_fn", "clusters_type"] and mod.BOOL_FLAGS == ["save_clusters"]
    assert mod.OPTIONAL_FLAGS == {"cluster_table": "anime", "n_clusters": 20, "cluster_iters": 50, "cluster_seed": 0,
                                  "cluster_top": 10, "cluster_query": None}
    assert C.CLUSTER_TABLES == ("anime", "user")
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    argv += ["--save_clusters", "True"]
    ns = parser.parse_args(argv)
    assert {f: getattr(ns, f) for f in mod.OPTIONAL_FLAGS} == mod.OPTIONAL_FLAGS and ns.save_clusters is True
    assert sorted(vars(ns)) == sorted(mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS))
    ns = parser.parse_args(argv + ["--cluster_table", " User", "--n_clusters", "4096", "--cluster_iters", "1000",
                                   "--cluster_seed", "7", "--cluster_top", "3", "--cluster_query", "Cowboy Bebop"])
    assert (ns.cluster_table, ns.n_clusters, ns.cluster_iters, ns.cluster_seed, ns.cluster_top, ns.cluster_query) == \
        ("user", 4096, 1000, 7, 3, "Cowboy Bebop")
    assert parser.parse_args(argv + ["--cluster_query", "none"]).cluster_query is None
    assert parser.parse_args(argv + ["--cluster_query", "5114"]).cluster_query == "5114"
    for bad in (["--cluster_table", "genre"], ["--n_clusters", "0"], ["--n_clusters", "4097"], ["--n_clusters", "2.5"],
                ["--n_clusters", "many"], ["--cluster_iters", "0"], ["--cluster_iters", "1001"], ["--cluster_seed", "-1"],
                ["--cluster_seed", "x"], ["--cluster_top", "0"], ["--save_clusters", "maybe"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    with pytest.raises(ValueError, match="anime, user"):        # the flags' own converters name what is allowed
        mod.cluster_table("genre")
    with pytest.raises(ValueError, match="1 .. 4096"):
        mod.n_clusters("4097")
    with pytest.raises(ValueError, match="1 .. 1000"):
        mod.cluster_iters("0")
    with pytest.raises(ValueError, match=">= 0"):
        mod.cluster_seed("-1")
    with pytest.raises(ValueError, match=">= 1"):
        mod.cluster_top("0")
    with pytest.raises(ValueError, match="anime, user"):
        C.cluster_table_name("both")
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "clusters", "MLproject")))
    assert ml["name"] == "clusters" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS)
    assert all(v["description"] for v in params.values()) and all(v["type"] == "str" for v in params.values())
    assert {k: v["default"] for k, v in params.items() if "default" in v} == \
        {"cluster_table": "anime", "n_clusters": "20", "cluster_iters": "50", "cluster_seed": "0", "cluster_top": "10",
         "cluster_query": "none"}
    for f, v in params.items():                                 # the MLproject defaults parse to the parser's own
        if "default" in v:
            assert getattr(mod, f)(v["default"]) == mod.OPTIONAL_FLAGS[f]
    assert main["command"] == "python clusters.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert yaml.safe_load(open(os.path.join(ROOT, "clusters", "conda.yml")))["name"] == "clusters"


def test_cluster_query_row_and_frames_on_the_host():
    """the frame builders are host code: fed with a hand-made fit they need no device (the user table's genres do)"""
    import pandas as pd
    import torch
    from anime_recommendations_amd import components as C
    anime_df = pd.DataFrame({"anime_id": [10, 20, 30, 40], "Name": ["a", "b", "c", "d"], "eng_version": ["a", "b", "c", "d"],
                             "Genres": ["Action, Comedy", "Action", "Drama", np.nan]})
    anime_ids, user_ids = np.array([30, 10, 20, 40, 50]), np.array([7, 8, 9])
    meta = C.metadata_by_index(anime_ids, anime_df)
    assert C.cluster_query_row("anime", "20", user_ids, anime_ids, anime_df) == 2
    assert C.cluster_query_row("anime", "a", user_ids, anime_ids, anime_df) == 1
    assert C.cluster_query_row("user", " 9 ", user_ids, anime_ids, anime_df) == 2
    with pytest.raises(ValueError, match="not a user id"):
        C.cluster_query_row("user", "bob", user_ids, anime_ids, anime_df)
    with pytest.raises(ValueError, match="not found|not in the model"):
        C.cluster_query_row("anime", "zzz", user_ids, anime_ids, anime_df)
    fit = dict(C=torch.zeros(3, 32), assign=torch.tensor([1, 0, 0, 1, -1], dtype=torch.int32),
               sim=torch.tensor([0.5, 0.25, 0.75, 0.5, float("nan")]))
    frame = C.clusters_frame(fit, "anime", anime_ids, meta, top=1)
    assert frame.columns.tolist() == C.CLUSTERS_COLUMNS and frame["size"].tolist() == [2, 2, 0]
    assert frame["top_members"].tolist() == ["b", "c", ""]       # nearest first; a tie to the lower row
    assert frame["top_genres"].tolist() == ["Action (2) | Comedy (1)", "Drama (1)", ""]
    assert frame["mean_similarity"].tolist()[:2] == [0.5, 0.5] and np.isnan(frame["mean_similarity"][2])
    assert C.clusters_frame(fit, "anime", anime_ids, meta, top=5)["top_members"][1] == "c | d"
    af = C.cluster_assignments_frame(fit, "anime", anime_ids)
    assert af.columns.tolist() == ["anime_id", "cluster", "similarity"] and af["cluster"].tolist() == [1, 0, 0, 1, -1]
    assert C.cluster_assignments_frame(fit, "user", anime_ids).columns[0] == "user_id"
    with pytest.raises(ValueError, match="top = 0"):
        C.clusters_frame(fit, "anime", anime_ids, meta, top=0)
    with pytest.raises(ValueError, match="5 assignments for a table of 3 ids"):
        C.clusters_frame(fit, "user", user_ids, meta)
