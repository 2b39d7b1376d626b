"""CPU tests of EASE: the NumPy restatement (tests/ease_restatement.py) held to numpy.linalg.inv by its residual and to
popularity on planted blocks; the library's symbols, size queries and refusals (no device is needed for them); the
names, flag surfaces and the ValueErrors that come before any GPU use.

The accuracy rule: the blocked Gauss-Jordan inverse's residual max |A P - I| is at most 8 x the larger of
numpy.linalg.inv's residual on the same A and n 2^-52.  The factor 8 is the project's ALS rule: it absorbs another
summation order, not another algorithm.  The rule holds for reg >= 1e-3 on the cases below and breaks at reg = 1e-6 on
a rank-deficient G (condition number 2.6e8): a reg far below 1 is outside the tested domain, and the header says so."""
import ctypes
import os
import re

import numpy as np
import pytest

import ease_cases as EC
import ease_restatement as R
from component_cli import load_component
from cooc_restatement import pack_bits
from test_cooc_cpu import _frames, _model, _table

from anime_recommendations_amd import _lib, build, components as C, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"anirec_spd_inverse_block": 0, "anirec_spd_inverse_workspace_bytes": 1, "anirec_spd_inverse": 7,
       "anirec_ease_weights": 6, "anirec_ease_scores_col_tile": 0, "anirec_ease_scores_entry_tile": 0,
       "anirec_ease_scores": 12}


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_users,reg", [(200, 500, 1.0), (333, 2000, 50.0), (257, 300, 1e-3), (1, 2, 1.0),
                                           (65, 130, 50.0)])
def test_blocked_inverse_meets_the_residual_rule(n, n_users, reg):
    bits, _ = EC.random_bits(n, n_users, n)
    A = R.gram_matrix(bits, n_users, reg)
    assert np.array_equal(A, A.T) and A[0, 0] == EC.random_bits(n, n_users, n)[1][0].sum() + reg
    P, info = R.spd_inverse(A)
    bound, ref = EC.residual_bound(A)
    res = R.residual(A, P)
    print("n = %d reg = %g: residual %.3g blocked, %.3g numpy, bound %.3g" % (n, reg, res, ref, bound))
    assert info == 0 and res <= bound
    for nb in (1, 7, n):                                                # the block size is no part of the mathematics
        Q, info = R.spd_inverse(A, nb)
        assert info == 0 and R.residual(A, Q) <= bound


def test_blocked_inverse_reports_the_first_bad_block():
    assert R.spd_inverse(-np.eye(65))[1] == 1
    A = EC.gram_case(130, 1.0)
    A[129, 129] = -1e9
    assert R.spd_inverse(A)[1] == 3
    assert R.spd_inverse(np.array([[np.nan]]))[1] == 1


def test_weights_and_scores_against_literal_loops():
    A = EC.gram_case(9, 2.0)
    P = np.linalg.inv(A)
    W = R.ease_weights(P)
    for i in range(9):
        for j in range(9):
            want = np.float32(0.0) if i == j else np.float32(-P[i, j] / P[j, j])
            assert W[i, j] == want and (i != j or not np.signbit(W[i, j]))
    off, hist, hw = np.asarray([0, 0, 3, 4]), np.asarray([2, 2, 5, 8]), np.asarray([0.5, 1.0, -2.0, 3.0], np.float32)
    got, err = R.ease_scores(W, off, hist, hw)
    assert err == 0 and not got[0].any()
    for l in range(3):
        for j in range(9):
            S = sum(int(np.rint(float(hw[e]) * float(W[hist[e], j]) * 2.0 ** 30)) for e in range(off[l], off[l + 1]))
            assert got[l, j] == np.float32(S * 2.0 ** -30)
    plain, _ = R.ease_scores(W, off, hist)
    assert np.array_equal(plain[2], np.float32(np.rint(W[8].astype(np.float64) * 2.0 ** 30) * 2.0 ** -30))
    # the flag: a bad item or term spares the rest, a bad pair is a NaN row
    bad, err = R.ease_scores(W, off, np.asarray([2, 9, 5, 8]), hw)
    assert err == 1 and np.array_equal(bad[2], got[2])
    assert np.array_equal(bad[1], R.ease_scores(W, [0, 2], [2, 5], hw[[0, 2]])[0][0])
    nan_row, err = R.ease_scores(W, [0, 3, 2, 4], hist, hw)
    assert err == 1 and np.isnan(nan_row[1]).all() and np.array_equal(nan_row[0], R.ease_scores(W, [0, 3], hist, hw)[0][0])
    big, err = R.ease_scores(W, [0, 1], [2], np.asarray([2000.0 / abs(W[2, 3])], np.float32))
    assert err == 1 and big[0, 3] == 0
    seen = np.zeros((3, 9), bool)
    seen[1, 0] = True
    assert R.ranks(got, seen, [1, 1], [0, 4]).tolist() == [int(np.sum(got[1, 1:] > got[1, 0])),
                                                           int(np.sum(np.delete(got[1], [0, 4]) > got[1, 4]))]


def test_planted_blocks_ease_beats_popularity():
    c = EC.planted()
    assert len(c["held_user"]) > 1400
    off, hist = EC.planted_histories(c)
    seen = c["B"][:, c["held_user"]].T
    pop = EC.popularity_hit_rate(c)
    for reg in (20.0, 100.0):
        W = R.ease_fit(pack_bits(c["B"]), c["n_users"], reg)
        scores, err = R.ease_scores(W, off, hist)
        hr = EC.hit_rate(R.ranks(scores, seen, np.arange(len(seen)), c["held_item"]))
        print("reg = %g: hit rate @10 %.4f, popularity %.4f" % (reg, hr, pop))
        assert err == 0 and hr > pop


# ---- the binding ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", code))
    for name, arity in NEW.items():
        assert name in declared and len(_lib.PROTOTYPES[name][1]) == arity, name
    assert "#define ANIREC_ABI_VERSION 5" in src and _lib.ABI_VERSION == 5
    assert "anirec_ease.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.anirec_abi_version() == 5
    assert "reg" in src and "not a knob" in src[src.index("anirec_spd_inverse:"):]


def test_size_queries_and_refusals_need_no_device():
    build.build(verbose=False)
    lib = _lib.load()
    nb = lib.anirec_spd_inverse_block()
    assert nb == R.NB and lib.anirec_ease_scores_col_tile() >= 256 and lib.anirec_ease_scores_entry_tile() >= 64
    assert lib.anirec_spd_inverse_workspace_bytes(0) == 0 and lib.anirec_spd_inverse_workspace_bytes(-3) == 0
    for n in (1, nb, nb + 1, 17560):
        pad = -(-n // nb) * nb
        assert lib.anirec_spd_inverse_workspace_bytes(n) == 8 * (nb * nb + 2 * nb * pad)
    fake = ctypes.c_void_p(4096)

    def inverse(A=fake, ld=10, n=10, info=fake, ws=fake, ws_bytes=1 << 20):
        return lib.anirec_spd_inverse(A, ld, n, info, ws, ws_bytes, None)
    assert inverse(n=0) == -1 and inverse(n=-1) == -1 and inverse(ld=9) == -1
    for name in ("A", "info", "ws"):
        assert inverse(**{name: None}) == -1, name
    assert inverse(A=ctypes.c_void_p(4100)) == -1 and inverse(ws=ctypes.c_void_p(4100)) == -1
    assert inverse(info=ctypes.c_void_p(4098)) == -1
    assert inverse(ws_bytes=lib.anirec_spd_inverse_workspace_bytes(10) - 1) == -3

    def weights(P=fake, ldp=10, n=10, W=fake, ldw=10):
        return lib.anirec_ease_weights(P, ldp, n, W, ldw, None)
    assert weights(n=0) == -1 and weights(ldp=9) == -1 and weights(ldw=9) == -1
    assert weights(P=None) == -1 and weights(W=None) == -1
    assert weights(P=ctypes.c_void_p(4100)) == -1 and weights(W=ctypes.c_void_p(4098)) == -1

    def scores(n_items=10, n_lists=3, n_hist=9, ldw=10, ld=10, p=fake, **null):
        a = dict(W=p, off=p, hi=p, out=p, err=p)
        a.update({k: None for k in null})
        return lib.anirec_ease_scores(a["W"], ldw, n_items, a["off"], a["hi"], None, n_lists, n_hist, a["out"], ld,
                                      a["err"], None)
    for kw in (dict(n_items=0), dict(n_lists=-1), dict(n_hist=-1), dict(ldw=9), dict(ld=9)):
        assert scores(**kw) == -1, kw
    assert scores(n_lists=0, p=None) == 0                               # no list: nothing enqueued or needed
    for name in ("W", "off", "hi", "out", "err"):
        assert scores(**{name: True}) == -1, name


def test_check_ease_needs_no_device():
    assert ops.check_ease(500, 0) == (500.0, 0) and ops.check_ease("2.5", "7") == (2.5, 7)
    for reg in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="reg"):
            ops.check_ease(reg, 0)
    with pytest.raises(ValueError, match="neighbours"):
        ops.check_ease(1.0, -1)


# ---- names, orderings and flag surfaces -------------------------------------------------------------------------------
def test_names_and_pinned_constants():
    assert recs.EASE_SYSTEMS == ("ease",) and C.LINEAR_BASELINES == ("ease",)
    assert C.EASE_DEFAULTS == {"reg": 500.0, "min_rating": 0.0, "neighbours": 0} and recs.EASE_REG == 500.0
    assert C.baseline_names("ease") == ("ease",)
    assert C.baseline_names(["ease", "content", "hybrid_tuned", "popularity", "als", "hybrid", "itemknn"]) == \
        ("popularity", "itemknn", "als", "hybrid", "hybrid_tuned", "content", "ease")
    with pytest.raises(ValueError, match="not supported.*hybrid_tuned, content, ease"):
        C.baseline_names("easy")
    assert recs.check_hybrid(("model", "Ease "))[0] == ("model", "ease")
    assert recs.check_hybrid(("ease", "content", "als"))[0] == ("ease", "content", "als")
    with pytest.raises(ValueError, match="not one of model, popularity, itemknn, als, content, ease"):
        recs.check_hybrid(("model", "easy"))
    # the pinned constants are as they were
    assert recs.HYBRID_SYSTEMS == ("model", "popularity", "itemknn", "als") and recs.CONTENT_SYSTEMS == ("content",)
    assert C.BASELINES == ("popularity", "itemknn") and C.FITTED_BASELINES == ("als",)
    assert C.FUSED_BASELINES == ("hybrid",) and C.TUNED_BASELINES == ("hybrid_tuned",)
    assert C.CONTENT_BASELINES == ("content",)
    assert list(C._systems()) == ["model", "popularity", "itemknn", "als", "content"]
    assert list(C._system_table()) == ["model", "popularity", "itemknn", "als", "content", "ease"]
    assert recs.ease_fit.__defaults__[:3] == (0.0, 500.0, 0)
    for doc in (recs.ease_fit.__doc__, C.evaluate_frame.__doc__):       # the default is documented as not tuned
        assert "not tuned on this data" in " ".join(doc.split())


def test_ease_recs_parser_and_mlproject_agree():
    mod = load_component("ease_recs")
    al = load_component("also_liked")
    assert mod.STR_FLAGS == al.STR_FLAGS and mod.BOOL_FLAGS == al.BOOL_FLAGS
    assert mod.OPTIONAL_FLAGS == {"user_query": "none", "ease_reg": 500.0, "ease_neighbours": 0, "liked_min_rating": 0.0}
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert {f: getattr(ns, f) for f in mod.OPTIONAL_FLAGS} == mod.OPTIONAL_FLAGS
    assert sorted(vars(ns)) == sorted(mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS))
    ns = parser.parse_args(argv + ["--user_query", " 42", "--ease_reg", "20", "--ease_neighbours", "30",
                                   "--liked_min_rating", "0.7"])
    assert (ns.user_query, ns.ease_reg, ns.ease_neighbours, ns.liked_min_rating) == ("42", 20.0, 30, 0.7)
    for bad in (["--user_query", "bob"], ["--ease_reg", "0"], ["--ease_reg", "-3"], ["--ease_reg", "inf"],
                ["--ease_reg", "x"], ["--ease_neighbours", "-1"], ["--ease_neighbours", "1.5"],
                ["--liked_min_rating", "1.5"], ["--save_sim_anime", "maybe"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "ease_recs", "MLproject")))
    assert ml["name"] == "ease_recs" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS)
    assert all(v["description"] for v in params.values())
    convert = dict(user_query=mod.user_query, ease_reg=mod.ease_reg, ease_neighbours=mod.ease_neighbours,
                   liked_min_rating=float)
    for f, v in params.items():
        if f in mod.OPTIONAL_FLAGS:
            assert convert[f](v["default"]) == mod.OPTIONAL_FLAGS[f]
        else:
            assert v["type"] == "str" and "default" not in v
    assert main["command"] == "python ease_recs.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert yaml.safe_load(open(os.path.join(ROOT, "ease_recs", "conda.yml")))["name"] == "ease_recs"
    # exactly one query
    none = [x if x != "x" or argv[i - 1] != "--anime_query" else "none" for i, x in enumerate(argv)]
    none = [x if x != "True" else "False" for x in none]
    with pytest.raises(ValueError, match="neither"):
        mod.query_of(parser.parse_args(none))
    with pytest.raises(ValueError, match="both"):
        mod.query_of(parser.parse_args(none + ["--user_query", "5", "--anime_query", "Naruto"]))
    assert mod.query_of(parser.parse_args(none + ["--user_query", "5"])) == ("user", 5)
    assert mod.query_of(parser.parse_args(none + ["--anime_query", "Naruto"])) == ("anime", "Naruto")
    assert mod.query_of(parser.parse_args(none + ["--random_anime", "True"])) == ("anime", None)


def test_evaluate_ease_flags_are_command_line_only():
    import yaml
    mod = load_component("evaluate")
    assert list(mod.EASE_FLAGS) == ["ease_reg", "ease_neighbours", "ease_min_rating"]
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    ns = mod.make_cli_parser().parse_args(argv)
    assert (ns.ease_reg, ns.ease_min_rating, ns.ease_neighbours) == (500.0, 0.0, 0)
    assert mod.ease_args(ns) == C.EASE_DEFAULTS
    ns = mod.make_cli_parser().parse_args(argv + ["--ease_reg", "20", "--ease_min_rating", "0.6", "--ease_neighbours", "9"])
    assert mod.ease_args(ns) == {"reg": 20.0, "min_rating": 0.6, "neighbours": 9}
    plain = mod.make_parser().parse_args(argv)
    assert not any(hasattr(plain, f) for f in mod.EASE_FLAGS) and mod.ease_args(plain) == {}
    ml = yaml.safe_load(open(os.path.join(ROOT, "evaluate", "MLproject")))
    params = ml["entry_points"]["main"]["parameters"]
    assert not set(params) & set(mod.EASE_FLAGS)
    assert list(params) == mod.STR_FLAGS + ["baseline"] + list(mod.OPTIONAL_FLAGS)      # the MLproject is as it was
    assert not any("--" + f + " " in ml["entry_points"]["main"]["command"] for f in mod.EASE_FLAGS)


# ---- ValueErrors before any GPU use -----------------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    """any use of the device fails the test"""
    def boom(*a, **kw):
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(ops, "_need_gpu", boom)
    monkeypatch.setattr(_lib, "call", boom)
    import torch
    monkeypatch.setattr(torch.Tensor, "cuda", boom)


def test_value_errors_come_before_any_gpu_use(no_gpu):
    table = _table()
    model = _model(table)
    for bad in (0, -5.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="reg"):
            C.evaluate_frame(model, table, 200, [1], 0.5, baseline="ease", ease={"reg": bad})
    with pytest.raises(ValueError, match="ease parameter"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="ease", ease={"lambda": 3})
    with pytest.raises(ValueError, match="neighbours"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline=["popularity", "ease"], ease={"neighbours": -2})
    with pytest.raises(ValueError, match="reg"):                        # as a hybrid member too
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="hybrid", hybrid={"systems": ("model", "ease")},
                         ease={"reg": 0})
    with pytest.raises(ValueError, match="reg"):
        recs.ease_fit([0], [0], [1.0], 1, 1, reg=0.0)
    with pytest.raises(ValueError, match="one entry per rating"):
        recs.ease_fit([0, 1], [0], [1.0], 2, 1)
    with pytest.raises(ValueError, match="neighbours"):
        recs.ease_fit([0], [0], [1.0], 1, 3, neighbours=5)
    df, anime_df, syn_df = _frames()
    with pytest.raises(ValueError, match="reg"):
        C.ease_recs_frame(df, anime_df, syn_df, 1000, 3, reg=-1.0)
    with pytest.raises(ValueError, match="no rating"):
        C.ease_recs_frame(df, anime_df, syn_df, 1, 3)
    with pytest.raises(ValueError, match="not found"):
        C.ease_similar_frame(df, anime_df, syn_df, "zzz", 3)
    with pytest.raises(ValueError, match="neighbours"):
        C.ease_similar_frame(df, anime_df, syn_df, "zzz", 3, neighbours=-1)
    ev = load_component("evaluate")
    eargv = []
    for f in ev.STR_FLAGS:
        eargv += ["--" + f, "x"]
    for extra in (["--baseline", "ease"], ["--baseline", "popularity,hybrid", "--hybrid_systems", "model,ease"]):
        with pytest.raises(ValueError, match="reg"):                    # before any file is opened
            ev.go(ev.make_cli_parser().parse_args(eargv + extra + ["--ease_reg", "0"]))
