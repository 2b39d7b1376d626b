"""CPU tests of the explained lists: the restatement's own rules on hand-built cases, the binding and the entry point's
refusals (no device needed), recs.history_csr, the ops checks and the explain_recs component's flag surface."""
import ctypes
import os

import numpy as np
import pytest

import explain_restatement as E
from component_cli import load_component

from anime_recommendations_amd import _lib, build, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = np.uint32(0x7FC00000)
INF = np.float32(np.inf)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- the restatement on hand-built cases ------------------------------------------------------------------------
def test_ties_go_to_the_lowest_position():
    S = np.array([[0.5, 0.25, 0.5, 0.5, 0.1]], np.float32)
    pos, sim, contrib = E.explain(S, np.full(5, 2.0, np.float32), [True], 3)
    assert pos.tolist() == [[0, 2, 3]] and contrib.tolist() == [[1.0, 1.0, 1.0]] and sim.tolist() == [[0.5, 0.5, 0.5]]
    pos, _, contrib = E.explain(S, np.array([1, 4, 1, 1, 5], np.float32), [True], 5)
    assert pos.tolist() == [[1, 0, 2, 3, 4]] and contrib.tolist() == [[1.0, 0.5, 0.5, 0.5, 0.5]]


def test_negative_zero_ties_with_positive_zero():
    S = np.array([[0.5, 0.5, 0.5, -0.5]], np.float32)
    w = np.array([-0.0, 0.0, -0.0, 0.0], np.float32)
    pos, sim, contrib = E.explain(S, w, [True], 4)
    assert pos.tolist() == [[0, 1, 2, 3]] and (contrib == 0).all()
    assert np.signbit(contrib[0]).tolist() == [True, False, True, True]    # the products keep their signs
    pos, _, _ = E.explain(S, np.array([0.0, -0.0, -1.0, -0.0], np.float32), [True], 4)
    assert pos.tolist() == [[0, 1, 3, 2]]                                   # (+0, -0, 0.5 > ... > -0.5)


def test_nan_is_never_picked_and_inf_comes_first():
    S = np.array([[0.5, np.nan, 0.0, 0.25, -0.5, 0.75]], np.float32)
    w = np.array([np.nan, 1.0, INF, INF, INF, 1.0], np.float32)     # NaN weight, NaN sim, 0 * inf, +inf, -inf
    pos, sim, contrib = E.explain(S, w, [True], 6)
    assert pos.tolist() == [[3, 5, 4, -1, -1, -1]]
    assert contrib[0, :3].tolist() == [np.inf, 0.75, -np.inf] and sim[0, :3].tolist() == [0.25, 0.75, -0.5]
    assert (_bits(contrib[0, 3:]) == NAN_BITS).all() and (_bits(sim[0, 3:]) == NAN_BITS).all()


def test_fewer_than_m_an_absent_slot_and_an_empty_history():
    S = np.array([[0.5, 0.25], [0.1, 0.9], [0.3, 0.3]], np.float32)
    pos, sim, contrib = E.explain(S, np.ones(2, np.float32), [True, False, True], 3)
    assert pos.tolist() == [[0, 1, -1], [-1, -1, -1], [0, 1, -1]]
    assert (_bits(sim[1]) == NAN_BITS).all() and (_bits(contrib[1]) == NAN_BITS).all()
    assert _bits(sim[0, 2]) == NAN_BITS and sim[2, :2].tolist() == [np.float32(0.3)] * 2
    pos, sim, contrib = E.explain(np.zeros((2, 0), np.float32), np.zeros(0, np.float32), [True, True], 2)
    assert (pos == -1).all() and (_bits(sim) == NAN_BITS).all() and (_bits(contrib) == NAN_BITS).all()


def test_explain_lists_cuts_the_histories_by_the_offsets():
    rng = np.random.default_rng(0)
    Sfull = rng.uniform(-1, 1, (9, 9)).astype(np.float32)
    idx = np.array([[1, -1, 4], [7, 7, 2], [-1, -1, -1]], np.int32)
    off = np.array([0, 4, 4, 7])
    hist = np.array([3, 8, 3, 0, 5, 6, 1], np.int32)
    w = rng.uniform(0.1, 1, 7).astype(np.float32)
    pos, sim, contrib = E.explain_lists(Sfull, idx, off, hist, w, 2)
    assert pos.shape == (3, 3, 2) and (pos[1] == -1).all() and (pos[2] == -1).all() and (pos[0, 1] == -1).all()
    c = w[:4] * Sfull[4, hist[:4]]
    assert pos[0, 2, 0] == int(np.argsort(-c, kind="stable")[0]) and contrib[0, 2, 0] == c.max()
    assert sim[0, 2, 0] == Sfull[4, hist[pos[0, 2, 0]]]


# ---- the binding, the limit queries and the entry point's refusals ----------------------------------------------
def test_symbols_declared_bound_and_exported():
    assert len(_lib.PROTOTYPES["anirec_explain_lists"][1]) == 15 and _lib.PROTOTYPES["anirec_explain_lists"][0] is ctypes.c_int
    assert len(_lib.PROTOTYPES["anirec_explain_max_k"][1]) == 1 and len(_lib.PROTOTYPES["anirec_explain_tile"][1]) == 2
    assert _lib.PROTOTYPES["anirec_explain_max_k"][0] is ctypes.c_size_t
    assert _lib.PROTOTYPES["anirec_explain_tile"][0] is ctypes.c_size_t
    assert _lib.ABI_VERSION == 5 and "anirec_explain.hip" in build.SOURCES and _lib.EXPLAIN_MAX_M == 8
    header = open(os.path.join(ROOT, "include", "anirec.h")).read()
    for name in ("anirec_explain_max_k", "anirec_explain_tile", "anirec_explain_lists"):
        assert name + "(" in header
    assert "#define ANIREC_EXPLAIN_MAX_M 8" in header and "#define ANIREC_ABI_VERSION 5" in header
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.anirec_abi_version() == 5
    for dim in _lib.WIDTHS:
        mk = lib.anirec_explain_max_k(dim)
        assert mk == _lib.explain_max_k(dim) and mk >= 64
        for k in (1, 2, 10, 33, 50, 64, mk):
            t = lib.anirec_explain_tile(dim, k)
            assert t == _lib.explain_tile(dim, k) and t >= 1
        assert lib.anirec_explain_tile(dim, 0) == 0 and lib.anirec_explain_tile(dim, -1) == 0
        assert lib.anirec_explain_tile(dim, mk + 1) == 0
    for dim in (0, 16, 48, 100, 512, -32):
        assert lib.anirec_explain_max_k(dim) == 0 and lib.anirec_explain_tile(dim, 10) == 0
        with pytest.raises(ValueError, match="embedding_size"):
            _lib.explain_max_k(dim)
    with pytest.raises(ValueError, match="1 .. 64 at width 256"):
        _lib.explain_tile(256, 65)


def test_entry_point_refuses_bad_arguments_without_a_device():
    build.build(verbose=False)
    lib = _lib.load()

    def call(dim=128, n_rows=50, n_lists=0, k=10, m=3, ptr=None, **null):
        p = {n: (None if null.get(n) else ptr) for n in ("What", "list_idx", "off", "hidx", "hw", "pos", "sim", "contrib", "err")}
        return lib.anirec_explain_lists(p["What"], dim, n_rows, p["list_idx"], n_lists, k, p["off"], p["hidx"], p["hw"], m,
                                        p["pos"], p["sim"], p["contrib"], p["err"], None)

    for dim in _lib.WIDTHS:
        mk = _lib.explain_max_k(dim)
        assert call(dim=dim) == 0 and call(dim=dim, k=mk, m=8) == 0 and call(dim=dim, k=1, m=1) == 0   # no lists: nothing to do
        assert call(dim=dim, k=mk + 1) == -1
    fake = 4096         # never followed: every refusal comes before anything is enqueued
    for kw in (dict(dim=48), dict(dim=0), dict(dim=512), dict(n_rows=0), dict(n_rows=-3), dict(n_lists=-1), dict(k=0),
               dict(k=-1), dict(k=129), dict(dim=256, k=65), dict(m=0), dict(m=9), dict(m=-1)):
        assert call(**kw) == -1, kw
        assert call(**dict(dict(n_lists=3, ptr=fake), **kw)) == -1, kw
    assert call(n_lists=3) == -1                                # NULL buffers with work to do
    for name in ("What", "list_idx", "off", "pos", "sim", "contrib", "err"):
        assert call(n_lists=3, ptr=fake, **{name: True}) == -1, name


# ---- recs.history_csr -------------------------------------------------------------------------------------------
def test_history_csr():
    user = np.array([2, 0, 2, 5, 0, 2, 5, 2])
    anime = np.array([10, 11, 12, 13, 14, 10, 16, 17])
    rating = np.array([0.7, 0.2, 0.9, 1.0, 0.7, 0.0, np.nan, 0.5])
    off, idx, r = recs.history_csr(user, anime, rating, [2, 0, 3, 5])
    assert off.dtype == np.int64 and idx.dtype == np.int32 and r.dtype == np.float32
    assert off.tolist() == [0, 4, 6, 6, 7]                      # user 3 has no ratings; user 5's NaN is dropped
    assert idx.tolist() == [10, 12, 10, 17, 11, 14, 13]         # the table's order within a user, a repeat kept
    assert r.tolist() == [np.float32(x) for x in (0.7, 0.9, 0.0, 0.5, 0.2, 0.7, 1.0)]
    off, idx, r = recs.history_csr(user, anime, rating.astype(np.float32), [2, 0, 3, 5], min_rating=0.7)
    assert off.tolist() == [0, 2, 3, 3, 4] and idx.tolist() == [10, 12, 14, 13]     # 0.7 itself is kept, in fp32
    off, idx, r = recs.history_csr(user, anime, rating, [0, 2, 0, 0])               # repeated users: the history again
    assert off.tolist() == [0, 2, 6, 8, 10] and idx.tolist() == [11, 14, 10, 12, 10, 17, 11, 14, 11, 14]
    off, idx, r = recs.history_csr(user, anime, rating, [])
    assert off.tolist() == [0] and len(idx) == 0 and len(r) == 0
    import torch
    off2, idx2, r2 = recs.history_csr(torch.from_numpy(user), torch.from_numpy(anime), torch.from_numpy(rating), [2, 0, 3, 5])
    assert off2.tolist() == [0, 4, 6, 6, 7] and idx2.tolist() == [10, 12, 10, 17, 11, 14, 13]
    with pytest.raises(ValueError, match="one entry per rating"):
        recs.history_csr(user, anime[:-1], rating, [0])


# ---- the ops checks ---------------------------------------------------------------------------------------------
def test_ops_refusals_need_no_gpu():
    import torch
    assert ops.check_explain(128, 10, 3) == (128, 10, 3) and ops.check_explain(256, 64, 8) == (256, 64, 8)
    with pytest.raises(ValueError, match="65 slots per list, 1 .. 64 at width 256"):
        ops.check_explain(256, 65, 3)
    with pytest.raises(ValueError, match="0 slots per list, 1 .. 128 at width 32"):
        ops.check_explain(32, 0, 3)
    for m in (0, 9, -1):
        with pytest.raises(ValueError, match=r"m = %d must be in 1 .. 8" % m):
            ops.check_explain(128, 10, m)
    with pytest.raises(ValueError, match="embedding_size"):
        ops.check_explain(48, 10, 3)
    What, li = torch.zeros(50, 128), torch.zeros(4, 10, dtype=torch.int32)
    with pytest.raises(ValueError, match="n_lists, k"):
        ops.explain_lists(What, li[0], [0], [], [], 3)
    with pytest.raises(ValueError, match="m = 9"):
        ops.explain_lists(What, li, [0, 0, 0, 0, 0], [], [], 9)
    with pytest.raises(ValueError, match="1 .. 128 at width 128"):
        ops.explain_lists(What, torch.zeros(4, 129, dtype=torch.int32), [0, 0, 0, 0, 0], [], [], 3)
    with pytest.raises(ValueError, match="not one of rating, similarity"):
        recs.explain_topk(What, li, [0, 0, 0, 0, 0], [], [], weight="both")


# ---- the component's flag surface -------------------------------------------------------------------------------
def test_explain_recs_parser_and_mlproject_agree():
    from anime_recommendations_amd import components as C
    mod, ref = load_component("explain_recs"), load_component("model_recs")
    assert mod.STR_FLAGS == ref.STR_FLAGS and mod.BOOL_FLAGS == ref.BOOL_FLAGS       # the model_recs flag set as it is
    assert mod.OPTIONAL_FLAGS == {"explain_count": 3, "explain_weight": "rating", "explain_min_rating": 0.0}
    assert C.EXPLAIN_WEIGHTS == recs.EXPLAIN_WEIGHTS == ("rating", "similarity") and C.EXPLAIN_MAX_COUNT == _lib.EXPLAIN_MAX_M
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert ns.explain_count == 3 and ns.explain_weight == "rating" and ns.explain_min_rating == 0.0
    assert sorted(vars(ns)) == sorted(ref.STR_FLAGS + ref.BOOL_FLAGS + ["explain_count", "explain_weight", "explain_min_rating"])
    ns = parser.parse_args(argv + ["--explain_count", "8", "--explain_weight", " Similarity", "--explain_min_rating", "0.7"])
    assert ns.explain_count == 8 and ns.explain_weight == "similarity" and ns.explain_min_rating == 0.7
    ns = parser.parse_args(argv + ["--explain_count", "1", "--explain_min_rating", "1"])
    assert ns.explain_count == 1 and ns.explain_min_rating == 1.0
    for bad in (["--explain_count", "0"], ["--explain_count", "9"], ["--explain_count", "2.5"], ["--explain_count", "many"],
                ["--explain_weight", "both"], ["--explain_min_rating", "-0.1"], ["--explain_min_rating", "1.5"],
                ["--explain_min_rating", "nan"], ["--explain_min_rating", "high"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    with pytest.raises(ValueError, match="1 .. 8"):             # the flags' own converters name what is allowed
        mod.explain_count("9")
    with pytest.raises(ValueError, match="rating, similarity"):
        mod.explain_weight("both")
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        mod.explain_min_rating("1.5")
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "explain_recs", "MLproject")))
    assert ml["name"] == "explain_recs" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    want = list(yaml.safe_load(open(os.path.join(ROOT, "model_recs", "MLproject")))["entry_points"]["main"]["parameters"])
    assert list(params) == want + ["explain_count", "explain_weight", "explain_min_rating"]
    assert all(v["description"] for v in params.values()) and all(v["type"] == "str" for v in params.values())
    assert {k: v["default"] for k, v in params.items() if "default" in v} == \
        {"explain_count": "3", "explain_weight": "rating", "explain_min_rating": "0.0"}
    assert main["command"] == "python explain_recs.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert yaml.safe_load(open(os.path.join(ROOT, "explain_recs", "conda.yml")))["name"] == "explain_recs"
