"""CPU tests of the RP3beta graph baseline: the NumPy restatement (tests/rp3_restatement.py) held to literal loops and
to popularity on planted blocks, and the cost of the 14-bit user weights measured against unquantised fp64 weights; the
library's symbols, size queries and refusals (no device is needed for them); the names, flag surfaces and the
ValueErrors that come before any GPU use."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import cooc_restatement as CR
import ease_cases as EC
import ease_restatement as ER
import rp3_cases as RC
import rp3_restatement as R
from component_cli import load_component
from test_cooc_cpu import _frames, _model, _table

from anime_recommendations_amd import _lib, build, components as C, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"anirec_wcooc_chunk_words": 0, "anirec_wcooc_workspace_bytes": 3, "anirec_wcooc_scores": 15}
GRID = list(itertools.product((0.5, 1.0), (0.0, 0.3, 0.6), (0, 50)))


# ---- the restatement --------------------------------------------------------------------------------------------------
def test_restatement_against_literal_loops():
    B, uq, q, row, col = RC.nine_items()
    assert set(uq.tolist()) <= set(RC.LIMB_VALUES) and len(set(q.tolist())) < len(q)
    w, S, ex, err = R.wcooc_scores(CR.pack_bits(B), B.shape[1], uq, q, row, col)
    lw, lS, lex = R.literal_wcooc(B, uq, q, row, col)
    assert err == 0 and S.any() and np.array_equal(S, lS)
    assert np.array_equal(w.view(np.uint32), lw.view(np.uint32)) and np.array_equal(CR.unpack_bits(ex, 9), lex)
    assert ex.shape == (len(q), 1) and not (ex >> np.uint32(9)).any()          # bits past n_items are clear
    # garbage past n_users changes nothing
    bits = CR.pack_bits(B)
    bits[:, -1] |= np.uint32(0xFFFFFF00)
    assert np.array_equal(R.wcooc_scores(bits, 40, uq, q, row, col)[1], S)
    # the flag: a bad query is a NaN row with sums of -1 and every bit, a bad weight counts as 0
    q2 = q.copy()
    q2[2] = 9
    w2, S2, ex2, err = R.wcooc_scores(CR.pack_bits(B), 40, uq, q2, row, col)
    assert err == 1 and np.isnan(w2[2]).all() and (S2[2] == -1).all() and ex2[2, 0] == 0x1FF
    keep = np.arange(len(q)) != 2
    assert np.array_equal(S2[keep], S[keep]) and np.array_equal(ex2[keep], ex[keep])
    uq2, uq3 = uq.copy(), uq.copy()
    uq2[[0, 7]], uq3[[0, 7]] = (-1, 16384), 0
    bad, zero = R.wcooc_scores(CR.pack_bits(B), 40, uq2, q, row, col), R.wcooc_scores(CR.pack_bits(B), 40, uq3, q, row, col)
    assert bad[3] == 1 and zero[3] == 0 and np.array_equal(bad[1], zero[1])


def test_user_weights_and_the_power_of_two():
    deg = np.asarray([0, 1, 2, 3, 10000, 7, 1])
    q = R.user_weights(deg, 1.0)
    assert q.tolist() == [0, 16383, 8192, 5461, 2, 2340, 16383]                 # 1.6383 rounds to 2: the coarse end
    assert np.array_equal(recs.rp3_user_weights(deg, 1.0), q) and q.dtype == np.int32
    assert R.user_weights([0, 5, 5], 0.5).tolist() == [0, 16383, 16383]         # relative to the lightest user
    assert R.user_weights([4, 10 ** 9], 1.0).tolist() == [16383, 1]             # never below 1 for a user with likes
    assert R.user_weights([3, 9], 0.0).tolist() == [16383, 16383] and R.user_weights([0, 0], 1.0).tolist() == [0, 0]
    for alpha in (0.5, 1.0, 2.0):
        d = np.random.default_rng(1).integers(0, 3000, 500)
        assert np.array_equal(recs.rp3_user_weights(d, alpha), R.user_weights(d, alpha))
    for m, want in ((256.0, 1.0), (511.9, 1.0), (512.0, 0.5), (255.9, 2.0), (1.0, 256.0), (3e-5, 2.0 ** 24)):
        assert float(R.pow2_scale(np.asarray([m, 0.0, np.nan], np.float32))) == want == recs._rp3_pow2(float(np.float32(m)))
        assert 256.0 <= np.float32(m) * np.float32(want) < 512.0
    assert float(R.pow2_scale([0.0])) == 1.0 == recs._rp3_pow2(0.0) and float(R.pow2_scale([])) == 1.0


def _hit_rate(fit, c, off, hist, seen):
    scores, err = R.rp3_scores(fit, off, hist)
    assert err == 0
    return EC.hit_rate(ER.ranks(scores, seen, np.arange(len(seen)), c["held_item"]))


def test_planted_blocks_rp3_beats_popularity_and_the_quantisation_costs_nothing():
    c = EC.planted()
    assert len(c["held_user"]) == 1455
    off, hist = EC.planted_histories(c)
    seen = c["B"][:, c["held_user"]].T
    pop = EC.popularity_hit_rate(c)
    for alpha, beta, neighbours in GRID:
        fit = R.rp3_fit(c["B"], alpha, beta, neighbours)
        top = np.nanmax(fit["W"] if "W" in fit else fit["nbr_sim"])
        assert 256.0 <= top < 512.0
        hr = _hit_rate(fit, c, off, hist, seen)
        exact = _hit_rate(R.rp3_fit(c["B"], alpha, beta, neighbours, quantised=False), c, off, hist, seen)
        print("alpha %.1f beta %.1f neighbours %2d: hit rate @10 %.4f with 14-bit user weights, %.4f with fp64 weights, "
              "popularity %.4f" % (alpha, beta, neighbours, hr, exact, pop))
        assert hr > pop
        assert round(hr, 4) == round(exact, 4)


# ---- the binding ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", code))
    for name, arity in NEW.items():
        assert name in declared and len(_lib.PROTOTYPES[name][1]) == arity, name
    assert "#define ANIREC_ABI_VERSION 5" in src and _lib.ABI_VERSION == 5
    assert "#define ANIREC_WCOOC_MAX_Q 16383" in src and _lib.WCOOC_MAX_Q == 16383 == recs.RP3_MAX_Q == R.MAX_Q
    assert "anirec_wcooc.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.anirec_abi_version() == 5


def test_size_queries_and_refusals_need_no_device():
    build.build(verbose=False)
    lib = _lib.load()
    chunk = 32 * lib.anirec_wcooc_chunk_words()
    assert chunk >= 64 and chunk % 64 == 0
    size = lib.anirec_wcooc_workspace_bytes
    assert size(0, 10, 1) == 0 and size(10, 0, 1) == 0 and size(10, 10, -1) == 0 and size(10, (1 << 24) + 1, 1) == 0
    for n_users in (1, chunk, chunk + 1, 350000, 1 << 24):
        assert size(17560, n_users, 1024) == 2 * (-(-n_users // chunk) * chunk)
    fake = ctypes.c_void_p(4096)

    def scores(n_items=10, n_users=100, nq=3, ws_bytes=1 << 20, **ptr):
        a = dict(bits=fake, uq=fake, q=fake, rs=None, cs=None, w=fake, sm=None, ex=None, err=fake, ws=fake)
        a.update(ptr)
        return lib.anirec_wcooc_scores(a["bits"], n_items, n_users, a["uq"], a["q"], nq, a["rs"], a["cs"], a["w"], a["sm"],
                                       a["ex"], a["err"], a["ws"], ws_bytes, None)
    for kw in (dict(n_items=0), dict(n_users=0), dict(nq=-1), dict(n_users=(1 << 24) + 1)):
        assert scores(**kw) == -1, kw
    assert scores(nq=0, bits=None, uq=None, q=None, w=None, err=None, ws=None) == 0     # no query: nothing enqueued
    for name in ("bits", "uq", "q", "w", "err", "ws"):
        assert scores(**{name: None}) == -1, name
    for name, addr in (("bits", 4098), ("uq", 4098), ("q", 4097), ("rs", 4100), ("cs", 4100), ("w", 4098), ("sm", 4100),
                       ("ex", 4098), ("err", 4098), ("ws", 4104)):
        assert scores(**{name: ctypes.c_void_p(addr)}) == -1, name
    assert scores(ws_bytes=size(10, 100, 3) - 1) == -3
    assert scores(n_users=1 << 24, ws_bytes=size(10, 1 << 24, 3) - 1) == -3            # 2^24 users pass the bound


def test_check_wcooc_needs_no_device():
    assert ops.check_wcooc(5, 9) == (5, 9) and ops.check_wcooc(1, 1 << 24) == (1, 1 << 24)
    assert ops.check_wcooc(3, 4, np.zeros(4, np.int32), np.ones(3), np.ones(3)) == (3, 4)
    for n_items, n_users, match in ((0, 5, "n_items"), (5, 0, "n_users"), (5, (1 << 24) + 1, "2\\^24")):
        with pytest.raises(ValueError, match=match):
            ops.check_wcooc(n_items, n_users)
    with pytest.raises(ValueError, match="user_q"):
        ops.check_wcooc(3, 4, np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="row_scale"):
        ops.check_wcooc(3, 4, None, np.ones(4))
    with pytest.raises(ValueError, match="col_scale"):
        ops.check_wcooc(3, 4, None, None, np.ones((3, 1)))
    assert recs.check_rp3("1", 0, "7") == (1.0, 0.0, 7)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            recs.check_rp3(bad, 0.3, 10)
        with pytest.raises(ValueError, match="beta"):
            recs.check_rp3(1.0, bad, 10)
    with pytest.raises(ValueError, match="neighbours"):
        recs.check_rp3(1.0, 0.3, -1)


# ---- names, orderings and flag surfaces -------------------------------------------------------------------------------
def test_names_and_pinned_constants():
    assert recs.GRAPH_SYSTEMS == ("rp3",) and C.GRAPH_BASELINES == ("rp3",)
    assert (recs.RP3_ALPHA, recs.RP3_BETA, recs.RP3_NEIGHBOURS) == (1.0, 0.3, 100)
    assert C.RP3_DEFAULTS == {"alpha": 1.0, "beta": 0.3, "neighbours": 100, "min_rating": 0.0}
    assert recs.rp3_fit.__defaults__[:4] == (0.0, 1.0, 0.3, 100)
    assert C.baseline_names("rp3") == ("rp3",)
    assert C.baseline_names(["rp3", "ease", "content", "hybrid_tuned", "popularity", "als", "hybrid", "itemknn"]) == \
        ("popularity", "itemknn", "als", "hybrid", "hybrid_tuned", "content", "ease", "rp3")
    with pytest.raises(ValueError, match="not supported.*hybrid_tuned, content, ease, rp3"):
        C.baseline_names("rp4")
    assert recs.check_hybrid(("model", "RP3 "))[0] == ("model", "rp3")
    assert recs.check_hybrid(("rp3", "ease", "als"))[0] == ("rp3", "ease", "als")
    with pytest.raises(ValueError, match="not one of model, popularity, itemknn, als, content, ease, rp3"):
        recs.check_hybrid(("model", "rp4"))
    # the pinned constants are as they were
    assert recs.HYBRID_SYSTEMS == ("model", "popularity", "itemknn", "als") and recs.CONTENT_SYSTEMS == ("content",)
    assert recs.EASE_SYSTEMS == ("ease",) and C.LINEAR_BASELINES == ("ease",)
    assert C.BASELINES == ("popularity", "itemknn") and C.FITTED_BASELINES == ("als",)
    assert C.FUSED_BASELINES == ("hybrid",) and C.TUNED_BASELINES == ("hybrid_tuned",)
    assert C.CONTENT_BASELINES == ("content",)
    assert list(C._systems()) == ["model", "popularity", "itemknn", "als", "content"]
    assert list(C._system_table()) == ["model", "popularity", "itemknn", "als", "content", "ease"]
    assert list(C._system_lookup()) == ["model", "popularity", "itemknn", "als", "content", "ease", "rp3"]
    assert recs.COOC_BATCH == 1024
    for doc in (recs.rp3_fit.__doc__, C.evaluate_frame.__doc__, C.rp3_similar_frame.__doc__):
        assert "not tuned on this data" in " ".join(doc.split())        # the defaults are documented as not tuned


def test_rp3_recs_parser_and_mlproject_agree():
    mod = load_component("rp3_recs")
    al = load_component("also_liked")
    assert mod.STR_FLAGS == al.STR_FLAGS and mod.BOOL_FLAGS == al.BOOL_FLAGS
    assert mod.OPTIONAL_FLAGS == {"user_query": "none", "rp3_alpha": 1.0, "rp3_beta": 0.3, "rp3_neighbours": 100,
                                  "liked_min_rating": 0.0}
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert {f: getattr(ns, f) for f in mod.OPTIONAL_FLAGS} == mod.OPTIONAL_FLAGS
    assert sorted(vars(ns)) == sorted(mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS))
    ns = parser.parse_args(argv + ["--user_query", " 42", "--rp3_alpha", "0.5", "--rp3_beta", "0", "--rp3_neighbours", "30",
                                   "--liked_min_rating", "0.7"])
    assert (ns.user_query, ns.rp3_alpha, ns.rp3_beta, ns.rp3_neighbours, ns.liked_min_rating) == ("42", 0.5, 0.0, 30, 0.7)
    for bad in (["--user_query", "bob"], ["--rp3_alpha", "-1"], ["--rp3_alpha", "inf"], ["--rp3_beta", "nan"],
                ["--rp3_beta", "x"], ["--rp3_neighbours", "-1"], ["--rp3_neighbours", "1.5"],
                ["--liked_min_rating", "1.5"], ["--save_sim_anime", "maybe"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "rp3_recs", "MLproject")))
    assert ml["name"] == "rp3_recs" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS)
    assert all(v["description"] for v in params.values())
    convert = dict(user_query=mod.user_query, rp3_alpha=mod.rp3_exponent, rp3_beta=mod.rp3_exponent,
                   rp3_neighbours=mod.rp3_neighbours, liked_min_rating=float)
    for f, v in params.items():
        if f in mod.OPTIONAL_FLAGS:
            assert convert[f](v["default"]) == mod.OPTIONAL_FLAGS[f]
        else:
            assert v["type"] == "str" and "default" not in v
    assert main["command"] == "python rp3_recs.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert yaml.safe_load(open(os.path.join(ROOT, "rp3_recs", "conda.yml")))["name"] == "rp3_recs"
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


def test_evaluate_rp3_flags_are_command_line_only():
    import yaml
    mod = load_component("evaluate")
    assert list(mod.RP3_FLAGS) == ["rp3_alpha", "rp3_beta", "rp3_neighbours", "rp3_min_rating"]
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    ns = mod.make_cli_parser().parse_args(argv)
    assert (ns.rp3_alpha, ns.rp3_beta, ns.rp3_neighbours, ns.rp3_min_rating) == (1.0, 0.3, 100, 0.0)
    assert mod.rp3_args(ns) == C.RP3_DEFAULTS
    ns = mod.make_cli_parser().parse_args(argv + ["--rp3_alpha", "0.5", "--rp3_beta", "0.6", "--rp3_neighbours", "9",
                                                  "--rp3_min_rating", "0.6"])
    assert mod.rp3_args(ns) == {"alpha": 0.5, "beta": 0.6, "neighbours": 9, "min_rating": 0.6}
    plain = mod.make_parser().parse_args(argv)
    assert not any(hasattr(plain, f) for f in mod.RP3_FLAGS) and mod.rp3_args(plain) == {}
    ml = yaml.safe_load(open(os.path.join(ROOT, "evaluate", "MLproject")))
    params = ml["entry_points"]["main"]["parameters"]
    assert not set(params) & set(mod.RP3_FLAGS)
    assert list(params) == mod.STR_FLAGS + ["baseline"] + list(mod.OPTIONAL_FLAGS)      # the MLproject is as it was
    assert list(mod.EASE_FLAGS) == ["ease_reg", "ease_neighbours", "ease_min_rating"]   # and so are the EASE flags


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
    for key in ("alpha", "beta"):
        for bad in (-5.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=key):
                C.evaluate_frame(model, table, 200, [1], 0.5, baseline="rp3", rp3={key: bad})
            with pytest.raises(ValueError, match=key):
                recs.rp3_fit([0], [0], [1.0], 1, 1, **{key: bad})
    with pytest.raises(ValueError, match="rp3 parameter"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="rp3", rp3={"gamma": 3})
    with pytest.raises(ValueError, match="neighbours"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline=["popularity", "rp3"], rp3={"neighbours": -2})
    with pytest.raises(ValueError, match="beta"):                       # as a hybrid member too
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="hybrid", hybrid={"systems": ("model", "rp3")},
                         rp3={"beta": -1})
    with pytest.raises(ValueError, match="one entry per rating"):
        recs.rp3_fit([0, 1], [0], [1.0], 2, 1, neighbours=0)
    with pytest.raises(ValueError, match="neighbours"):
        recs.rp3_fit([0], [0], [1.0], 1, 3, neighbours=5)
    with pytest.raises(ValueError, match="neighbours"):
        recs.rp3_fit([0], [0], [1.0], 1, 3, neighbours=-1)
    with pytest.raises(ValueError, match="n_users"):
        recs.rp3_fit([0], [0], [1.0], (1 << 24) + 1, 3, neighbours=1)
    df, anime_df, syn_df = _frames()
    with pytest.raises(ValueError, match="alpha"):
        C.rp3_recs_frame(df, anime_df, syn_df, 1000, 3, alpha=-1.0)
    with pytest.raises(ValueError, match="no rating"):
        C.rp3_recs_frame(df, anime_df, syn_df, 1, 3)
    with pytest.raises(ValueError, match="not found"):
        C.rp3_similar_frame(df, anime_df, syn_df, "zzz", 3)
    with pytest.raises(ValueError, match="neighbours"):
        C.rp3_similar_frame(df, anime_df, syn_df, "zzz", 3, neighbours=-1)
    ev = load_component("evaluate")
    eargv = []
    for f in ev.STR_FLAGS:
        eargv += ["--" + f, "x"]
    for extra in (["--baseline", "rp3"], ["--baseline", "popularity,hybrid", "--hybrid_systems", "model,rp3"]):
        with pytest.raises(ValueError, match="beta"):                   # before any file is opened
            ev.go(ev.make_cli_parser().parse_args(eargv + extra + ["--rp3_beta", "-1"]))
