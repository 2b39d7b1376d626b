"""CPU tests of the content-based system: the restatement against literal Python loops, ``content_fit`` against
hand-computed TF-IDF, the binding and the entry point's refusals (no device needed), the ValueErrors that come before
any GPU use, the flag surfaces, and the host logic of recs / components with ``ops`` replaced by the restatement."""
import ctypes
import math
import os
import re
import struct

import numpy as np
import pandas as pd
import pytest

import content_restatement as R
import cooc_restatement as CR
from component_cli import load_component
from test_cooc_cpu import _frames, _model, _table, host_ops as cooc_host_ops  # noqa: F401

from anime_recommendations_amd import _lib, build, components as C, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"anirec_content_lds_tokens": 0, "anirec_content_workspace_bytes": 2, "anirec_content_scores": 15}


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _fma32(a, b, c):
    """fp32 fma from exact rational arithmetic: the yardstick of the yardstick"""
    from fractions import Fraction
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return _round32(exact)


def _round32(q):
    """the fp32 nearest a Fraction, ties to even (finite, normal range or zero)"""
    if q == 0:
        return 0.0
    lo = float(np.float32(float(q)))            # near enough to find the neighbours
    cands = {lo, float(np.nextafter(np.float32(lo), np.float32(np.inf))), float(np.nextafter(np.float32(lo), np.float32(-np.inf)))}
    from fractions import Fraction
    best = sorted(cands, key=lambda c: (abs(Fraction(c) - q), int(np.float32(c).view(np.uint32)) & 1))
    return best[0]


# ---- the restatement against literal loops ----------------------------------------------------------------------------
def _small_csr():
    # item 2 is empty, item 3 repeats token 1, item 4 holds a weight that is no multiple of 2^-30
    rows = [[(0, 0.5), (2, 0.75)], [(1, 1.0)], [], [(1, 0.25), (1, 0.5), (3, 0.125)], [(0, 0.1), (3, 0.3)]]
    off = np.cumsum([0] + [len(r) for r in rows])
    idx = np.asarray([v for r in rows for v, _ in r], np.int32)
    w = np.asarray([x for r in rows for _, x in r], np.float32)
    return rows, off, idx, w


def test_restatement_equals_literal_loops():
    from fractions import Fraction
    rows, off, idx, w = _small_csr()
    hoff = [0, 3, 3, 6, 8, 10]
    hidx = [0, 4, 4, 1, 3, 2, 0, 1, 4, 3]
    hw = np.asarray([1.0, 0.3, 0.3, 0.7, -0.4, 2.0, 0.0, 0.0, 0.5, -0.5], np.float32)
    for weights in (None, hw):
        out, err = R.content_scores(off, idx, w, 4, hoff, hidx, weights)
        assert err == 0 and out.shape == (5, 5)
        for l in range(5):
            P, Wq = [0] * 4, 0
            for e in range(hoff[l], hoff[l + 1]):
                we = 1.0 if weights is None else float(weights[e])
                Wq += round(abs(we) * 2.0 ** 30)                                # half-even, as llrint
                for v, x in rows[hidx[e]]:
                    P[v] += round(we * float(np.float32(x)) * 2.0 ** 30)
            p = [_round32(Fraction(float(P[v]) / float(Wq))) if Wq > 0 else 0.0 for v in range(4)]
            for j, r in enumerate(rows):
                acc = 0.0
                for v, x in r:
                    acc = _fma32(p[v], np.float32(x), acc)
                assert out[l, j] == acc and not (acc == 0.0 and np.signbit(out[l, j]) and not r), (l, j)
        assert (out[1] == 0).all() and not np.signbit(out[1]).any()            # an empty history
        assert (out[:, 2] == 0).all() and not np.signbit(out[:, 2]).any()      # an item without tokens: +0
    out, _ = R.content_scores(off, idx, w, 4, hoff, hidx, hw)
    assert (out[3] == 0).all() and not np.signbit(out[3]).any()                # all-zero weights: Wq = 0, a zero row
    assert (out[4] != 0).any()                                                 # weights that cancel in Wq's sign only
    # a repeated item counts again, in P and in Wq alike: the mean does not move
    twice, _ = R.content_scores(off, idx, w, 4, [0, 2], [0, 0], [1.0, 1.0])
    once, _ = R.content_scores(off, idx, w, 4, [0, 1], [0], [1.0])
    assert twice.tobytes() == once.tobytes()
    # entry order inside a list changes nothing
    perm = [2, 0, 1, 5, 4, 3, 7, 6, 9, 8]
    again, _ = R.content_scores(off, idx, w, 4, hoff, np.asarray(hidx)[perm], hw[perm])
    assert again.tobytes() == R.content_scores(off, idx, w, 4, hoff, hidx, hw)[0].tobytes()
    ones, _ = R.content_scores(off, idx, w, 4, hoff, hidx, np.ones(10, np.float32))
    assert ones.tobytes() == R.content_scores(off, idx, w, 4, hoff, hidx, None)[0].tobytes()


def test_restatement_bad_values_raise_the_flag_and_spare_the_other_lists():
    rows, off, idx, w = _small_csr()
    hoff, hidx = [0, 3, 5, 7], [0, 4, 1, 3, 0, 4, 1]
    hw = np.asarray([1.0, 0.3, 0.7, -0.4, 2.0, 0.5, 0.25], np.float32)
    good, err = R.content_scores(off, idx, w, 4, hoff, hidx, hw)
    assert err == 0
    for what in ("item", "offsets", "nan", "inf", "large", "heavy"):
        hoff2, hidx2, hw2 = list(hoff), list(hidx), hw.copy()
        if what == "item":
            hidx2[3] = 5
        elif what == "offsets":
            hoff2[2] = 2                                 # list 1 is (3, 2): decreasing; list 2 becomes (2, 7)
        elif what == "nan":
            hw2[3] = np.nan
        elif what == "inf":
            hw2[3] = np.inf
        elif what == "large":
            hw2[3] = 1024.5                              # the entry itself is past the range
        else:
            hw2[3] = -1000.0                             # usable alone, unusable against no token here: no flag
        out, err = R.content_scores(off, idx, w, 4, hoff2, hidx2, hw2)
        assert err == (0 if what == "heavy" else 1), what
        assert out[0].tobytes() == good[0].tobytes(), what
        if what == "offsets":
            assert (_u32(out[1]) == 0x7FC00000).all()
        else:
            assert out[2].tobytes() == good[2].tobytes(), what
            if what != "heavy":                          # the entry is dropped, from Wq too: list 1 is entry 4 alone
                alone, _ = R.content_scores(off, idx, w, 4, [0, 1], [0], [2.0])
                assert out[1].tobytes() == alone[0].tobytes(), what
    # a bad token slot is skipped in the profile and in the chain: the call with that slot's weight 0 and id 0
    for what in ("token", "token_nan"):
        idx2, w2, idx3, w3 = idx.copy(), w.copy(), idx.copy(), w.copy()
        if what == "token":
            idx2[4] = 4
        else:
            w2[4] = np.nan
        idx3[4], w3[4] = 0, 0.0
        out, err = R.content_scores(off, idx2, w2, 4, hoff, hidx, hw)
        clean, err3 = R.content_scores(off, idx3, w3, 4, hoff, hidx, hw)
        assert err == 1 and err3 == 0 and out.tobytes() == clean.tobytes(), what
    # a term past the range: 1000 x 2.0
    w4 = w.copy()
    w4[2] = 2.0                                          # item 1's only token
    out, err = R.content_scores(off, idx, w4, 4, [0, 2, 3], [1, 0, 0], [1000.0, 1.0, 1.0])
    assert err == 1
    assert out[1].tobytes() == R.content_scores(off, idx, w4, 4, [0, 1], [0], [1.0])[0].tobytes()


# ---- content_fit against hand-computed TF-IDF -------------------------------------------------------------------------
def _meta():
    return pd.DataFrame({
        "Genres": ["Action, Comedy", "Action", np.nan, "Comedy, Manga", "Action", "Drama"],
        "Type": ["TV", "TV", np.nan, "Movie", "OVA", "TV"],
        "Source": ["Manga", "Original", np.nan, "Manga", "Manga", "Original"],
        "Studios": ["A", "A, B", np.nan, "B", "A", "C"],
        "Rating": ["PG", "PG", np.nan, "R", "PG", "R"],
        "Sypnopsis": ["A robot fights. The robot wins, robot!", "Two friends and a robot", np.nan, "None",
                      "friends at school", "an old school of robot friends at it"]})


def test_content_fit_against_hand_computed_tfidf():
    meta = _meta()
    fit = recs.content_fit(meta, ("Genres", "Source"), device="cpu")
    assert fit["vocab"] == ["Genres=Action", "Genres=Comedy", "Genres=Drama", "Genres=Manga", "Source=Manga",
                            "Source=Original"]                          # sorted; Manga is two tokens, one per column
    assert fit["n_items"] == 6 and fit["n_tokens"] == 6 and fit["columns"] == ("Genres", "Source")
    off, idx, w = (fit[k].numpy() for k in ("tok_offsets", "tok_idx", "tok_w"))
    assert off.dtype == np.int64 and idx.dtype == np.int32 and w.dtype == np.float32
    assert off.tolist() == [0, 3, 5, 5, 8, 10, 12]                     # the NaN row is empty
    assert idx.tolist() == [0, 1, 4, 0, 5, 1, 3, 4, 0, 4, 2, 5]        # ascending within a row
    df = {0: 3, 1: 2, 2: 1, 3: 1, 4: 3, 5: 2}
    idf = {v: math.log(7.0 / (1 + d)) + 1.0 for v, d in df.items()}
    for j in range(6):
        raw = [idf[int(v)] for v in idx[off[j]:off[j + 1]]]            # tf = 1
        norm = math.sqrt(math.fsum(x * x for x in raw))
        assert w[off[j]:off[j + 1]].tolist() == [_f32(x / norm) for x in raw]
        if raw:
            assert abs(float(np.sum(w[off[j]:off[j + 1]].astype(np.float64) ** 2)) - 1.0) < 1e-6
    # the synopsis: lower-cased, [a-z]{3,}, tf = 1 + ln(count), and the df filter on these tokens alone
    syn = recs.content_fit(meta, ("Type", "Sypnopsis"), device="cpu")
    assert "Sypnopsis=robot" in syn["vocab"] and "Sypnopsis=at" not in syn["vocab"] and "Sypnopsis=none" not in syn["vocab"]
    assert "Sypnopsis=the" in syn["vocab"] and "Type=TV" in syn["vocab"]
    o, i, x = (syn[k].numpy() for k in ("tok_offsets", "tok_idx", "tok_w"))
    v = syn["vocab"]
    n_doc = {t: sum(1 for c in meta["Sypnopsis"] if isinstance(c, str) and c != "None" and
                    t in re.findall(r"[a-z]{3,}", c.lower())) for t in ("robot", "fights", "the", "wins")}
    assert n_doc == {"robot": 3, "fights": 1, "the": 1, "wins": 1}
    raw = {"Type=TV": 1.0 * (math.log(7 / 4) + 1), "Sypnopsis=robot": (1 + math.log(3)) * (math.log(7 / 4) + 1),
           "Sypnopsis=fights": math.log(7 / 2) + 1, "Sypnopsis=the": math.log(7 / 2) + 1, "Sypnopsis=wins": math.log(7 / 2) + 1}
    norm = math.sqrt(math.fsum(a * a for a in raw.values()))
    row0 = {v[int(t)]: float(c) for t, c in zip(i[o[0]:o[1]], x[o[0]:o[1]])}
    assert row0 == {t: _f32(a / norm) for t, a in raw.items()}
    assert o[4] - o[3] == 1                                            # "None" is no synopsis: the Type token alone
    cut = recs.content_fit(meta, ("Type", "Sypnopsis"), min_df=2, max_df=0.4, device="cpu")
    words = sorted(t for t in cut["vocab"] if t.startswith("Sypnopsis="))
    assert words == ["Sypnopsis=school"]                               # df 2 = floor(0.4 * 6); robot and friends have 3
    assert [t for t in cut["vocab"] if t.startswith("Type=")] == ["Type=Movie", "Type=OVA", "Type=TV"]   # not filtered
    # the restatement's TF-IDF is the same arrays
    for cols, kw in ((("Genres", "Source"), {}), (("Type", "Sypnopsis"), dict(min_df=2, max_df=0.4)),
                     (recs.CONTENT_COLUMNS, {})):
        f = recs.content_fit(meta, cols, device="cpu", **kw)
        vocab, ro, ri, rw = R.tfidf({c: meta[c].tolist() for c in cols}, **kw)
        assert f["vocab"] == vocab and f["tok_offsets"].numpy().tolist() == ro.tolist()
        assert f["tok_idx"].numpy().tolist() == ri.tolist() and f["tok_w"].numpy().tobytes() == rw.tobytes()
    empty = recs.content_fit(meta.iloc[[2]], device="cpu")
    assert empty["n_tokens"] == 1 and empty["vocab"] == [] and empty["tok_offsets"].tolist() == [0, 0]


def test_content_history_weights():
    r = np.asarray([0.5, 0.7, 0.9, 0.2, 0.4], np.float32)
    assert recs.content_history_weights(r, "rating").tobytes() == r.tobytes()
    assert recs.content_history_weights(r, " One ").tolist() == [1.0] * 5
    c = recs.content_history_weights(r, "centered", [0, 3, 3, 5])
    assert c.dtype == np.float32
    assert c.tolist() == (r[:3] - r[:3].mean(dtype=np.float32)).tolist() + (r[3:] - r[3:].mean(dtype=np.float32)).tolist()
    assert recs.content_history_weights(r, "centered").tolist() == (r - r.mean(dtype=np.float32)).tolist()
    assert recs.CONTENT_WEIGHTS == ("rating", "centered", "one")
    with pytest.raises(ValueError, match="rating, centered, one"):
        recs.content_history_weights(r, "mean")


# ---- the binding ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", code))
    for name, arity in NEW.items():
        assert name in declared and len(_lib.PROTOTYPES[name][1]) == arity, name
    assert "#define ANIREC_ABI_VERSION 5" in src and _lib.ABI_VERSION == 5
    assert "anirec_content.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.anirec_abi_version() == 5


def test_size_queries_and_refusals_need_no_device():
    build.build(verbose=False)
    lib = _lib.load()
    lds = lib.anirec_content_lds_tokens()
    assert lds >= 12 * 1024 and lds * 8 <= 160 * 1024
    assert lib.anirec_content_workspace_bytes(0, 5) == 0 and lib.anirec_content_workspace_bytes(10, -1) == 0
    assert 0 < lib.anirec_content_workspace_bytes(lds, 5) < lds * 8
    assert lib.anirec_content_workspace_bytes(lds + 1, 5) == (lds + 1) * 5 * 8
    assert 0 < lib.anirec_content_workspace_bytes(lds + 1, 0) <= 256
    fake = ctypes.c_void_p(4096)

    def call(n_items=10, n_tokens=4, n_lists=3, n_hist=9, p=fake, ws_bytes=1 << 20, **null):
        a = dict(to=p, ti=p, tw=p, off=p, hi=p, out=p, err=p, ws=p)
        a.update({k: None for k in null})
        return lib.anirec_content_scores(a["to"], a["ti"], a["tw"], n_items, n_tokens, a["off"], a["hi"], None, n_lists,
                                         n_hist, a["out"], a["err"], a["ws"], ws_bytes, None)
    for kw in (dict(n_items=0), dict(n_tokens=0), dict(n_lists=-1), dict(n_hist=-1)):
        assert call(**kw) == -1, kw
        assert call(**dict(kw, n_lists=0)) == -1 or "n_lists" in kw, kw        # refused whatever else the call holds
    assert call(n_lists=0, p=None) == 0                                        # no list: nothing enqueued or needed
    for name in ("to", "ti", "tw", "off", "hi", "out", "err", "ws"):
        assert call(**{name: True}) == -1, name
    assert call(n_tokens=lds + 1, ws_bytes=(lds + 1) * 3 * 8 - 1) == -3
    assert call(ws_bytes=255) == -3


def test_ops_check_content_needs_no_device():
    off, idx, w = np.zeros(4, np.int64), np.zeros(5, np.int32), np.zeros(5, np.float32)
    assert ops.check_content(off, idx, w, 7) == (3, 7, 5)
    with pytest.raises(ValueError, match="n_items"):
        ops.check_content(off[:1], idx, w, 7)
    with pytest.raises(ValueError, match="one entry per token slot"):
        ops.check_content(off, idx, w[:4], 7)
    with pytest.raises(ValueError, match="n_tokens"):
        ops.check_content(off, idx, w, 0)
    with pytest.raises(ValueError, match="n_tokens"):                           # before the device is asked for
        ops.content_scores(off, idx, w, 0, [0], [])


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
    meta = _meta()
    for cols in (("Genres", "Score"), (), ("Genres", "Genres"), "Name"):
        with pytest.raises(ValueError, match="content column"):
            recs.check_content_fit(cols)
    for kw in (dict(min_df=0), dict(max_df=0.0), dict(max_df=1.5)):
        with pytest.raises(ValueError, match="min_df"):
            recs.content_fit(meta, **kw)
    with pytest.raises(ValueError, match="no column"):
        recs.content_fit(meta.drop(columns=["Studios"]))
    df, anime_df, syn_df = _frames()
    with pytest.raises(ValueError, match="content column"):
        C.content_similar_frame(anime_df, syn_df, "a", 3, columns=["Genres", "Members"])
    with pytest.raises(ValueError, match="content_weight"):
        C.content_recs_frame(df, anime_df, syn_df, 1000, 3, weight="squared")
    with pytest.raises(ValueError, match="content column"):
        C.content_recs_frame(df, anime_df, syn_df, 1000, 3, columns=["genres"])
    with pytest.raises(ValueError, match="no rating"):
        C.content_recs_frame(df, anime_df, syn_df, 1, 3)
    with pytest.raises(ValueError, match="not found"):
        C.content_similar_frame(anime_df, syn_df, "zzz", 3)
    table = _table()
    model = _model(table)
    with pytest.raises(ValueError, match="metadata"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="content")
    with pytest.raises(ValueError, match="metadata"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="hybrid", hybrid={"systems": ("model", "content")})
    with pytest.raises(ValueError, match="content_weight"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="content", content={"meta": meta, "weight": "x"})
    with pytest.raises(ValueError, match="content parameter"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="content", content={"meta": meta, "k": 3})
    with pytest.raises(ValueError, match="content column"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="content", content={"meta": meta, "columns": ("x",)})
    # the components' own checks
    mod = load_component("content_recs")
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "none" if f == "anime_query" else "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "False"]
    parser = mod.make_parser()
    with pytest.raises(ValueError, match="neither"):
        mod.go(parser.parse_args(argv))
    with pytest.raises(ValueError, match="both"):
        mod.go(parser.parse_args(argv + ["--user_query", "5", "--anime_query", "Naruto"]))
    with pytest.raises(ValueError, match="both"):
        mod.go(parser.parse_args(argv + ["--user_query", "5", "--random_anime", "True"]))
    assert mod.query_of(parser.parse_args(argv + ["--user_query", "5"])) == ("user", 5)
    assert mod.query_of(parser.parse_args(argv + ["--anime_query", "Naruto"])) == ("anime", "Naruto")
    assert mod.query_of(parser.parse_args(argv + ["--random_anime", "True"])) == ("anime", None)
    ev = load_component("evaluate")
    eargv = []
    for f in ev.STR_FLAGS:
        eargv += ["--" + f, "x"]
    for extra in (["--baseline", "content"], ["--baseline", "popularity,hybrid", "--hybrid_systems", "model,content"]):
        with pytest.raises(ValueError, match="--anime_df"):
            ev.go(ev.make_cli_parser().parse_args(eargv + extra))
        with pytest.raises(ValueError, match="--anime_df"):                    # the MLproject's parser has no such flag
            ev.go(ev.make_parser().parse_args(eargv + extra[:2]) if len(extra) == 2 else
                  ev.make_cli_parser().parse_args(eargv + extra))
    with pytest.raises(ValueError, match="content_weight"):
        ev.go(ev.make_cli_parser().parse_args(eargv + ["--baseline", "content", "--anime_df", "a:latest",
                                                       "--content_weight", "x"]))
    with pytest.raises(ValueError, match="content column"):
        ev.go(ev.make_cli_parser().parse_args(eargv + ["--baseline", "content", "--anime_df", "a:latest",
                                                       "--content_columns", "Genres,Nope"]))
    assert not ev.wants_content(ev.make_cli_parser().parse_args(eargv + ["--hybrid_systems", "model,content"]))


# ---- the flag surfaces ------------------------------------------------------------------------------------------------
def test_content_recs_parser_and_mlproject_agree():
    mod = load_component("content_recs")
    al = load_component("also_liked")
    assert mod.STR_FLAGS == al.STR_FLAGS and mod.BOOL_FLAGS == al.BOOL_FLAGS
    assert mod.OPTIONAL_FLAGS == {"user_query": "none", "content_columns": "Genres,Type,Source,Studios,Rating",
                                  "content_weight": "rating", "content_min_rating": 0.0}
    assert mod.CONTENT_WEIGHTS == recs.CONTENT_WEIGHTS and mod.KNOWN_COLUMNS == recs.CONTENT_COLUMNS + (recs.CONTENT_SYNOPSIS,)
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert {f: getattr(ns, f) for f in mod.OPTIONAL_FLAGS} == mod.OPTIONAL_FLAGS
    assert sorted(vars(ns)) == sorted(mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS))
    ns = parser.parse_args(argv + ["--user_query", " 42", "--content_columns", "Genres, Sypnopsis", "--content_weight",
                                   " Centered", "--content_min_rating", "0.7"])
    assert (ns.user_query, ns.content_columns, ns.content_weight, ns.content_min_rating) == \
        ("42", "Genres,Sypnopsis", "centered", 0.7)
    for bad in (["--user_query", "bob"], ["--content_columns", "Genres,Score"], ["--content_columns", ""],
                ["--content_columns", "Type,Type"], ["--content_weight", "mean"], ["--content_min_rating", "1.5"],
                ["--content_min_rating", "x"], ["--save_sim_anime", "maybe"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "content_recs", "MLproject")))
    assert ml["name"] == "content_recs" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS)
    assert all(v["description"] for v in params.values())
    for f, v in params.items():
        if f in mod.OPTIONAL_FLAGS:
            assert getattr(mod, f)(v["default"]) == mod.OPTIONAL_FLAGS[f]
        else:
            assert v["type"] == "str" and "default" not in v
    assert main["command"] == "python content_recs.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert yaml.safe_load(open(os.path.join(ROOT, "content_recs", "conda.yml")))["name"] == "content_recs"


def test_evaluate_content_flags_are_command_line_only():
    import yaml
    mod = load_component("evaluate")
    assert list(mod.CONTENT_FLAGS) == ["anime_df", "anime_df_type", "sypnopses_df", "sypnopsis_df_type", "content_columns",
                                       "content_weight", "content_min_rating"]
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    ns = mod.make_cli_parser().parse_args(argv)
    assert (ns.anime_df, ns.sypnopses_df, ns.content_weight, ns.content_min_rating) == ("none", "none", "rating", 0.0)
    assert ns.content_columns.split(",") == list(C.CONTENT_DEFAULTS["columns"])
    assert not any(hasattr(mod.make_parser().parse_args(argv), f) for f in mod.CONTENT_FLAGS)
    ml = yaml.safe_load(open(os.path.join(ROOT, "evaluate", "MLproject")))
    params = ml["entry_points"]["main"]["parameters"]
    assert not set(params) & set(mod.CONTENT_FLAGS)
    assert list(params) == mod.STR_FLAGS + ["baseline"] + list(mod.OPTIONAL_FLAGS)      # the MLproject is as it was
    assert not any("--" + f + " " in ml["entry_points"]["main"]["command"] for f in mod.CONTENT_FLAGS)


def test_names_and_pinned_constants():
    assert recs.CONTENT_SYSTEMS == ("content",) and C.CONTENT_BASELINES == ("content",)
    assert C.CONTENT_COLUMNS == recs.CONTENT_COLUMNS == ("Genres", "Type", "Source", "Studios", "Rating")
    assert C.CONTENT_DEFAULTS == {"columns": recs.CONTENT_COLUMNS, "weight": "rating", "min_rating": 0.0, "min_df": 1,
                                  "max_df": 1.0}
    assert recs.CONTENT_BATCH == 4096
    assert C.baseline_names("content") == ("content",)
    assert C.baseline_names(["content", "hybrid_tuned", "popularity", "als", "hybrid", "itemknn"]) == \
        ("popularity", "itemknn", "als", "hybrid", "hybrid_tuned", "content")
    with pytest.raises(ValueError, match="not supported.*popularity, itemknn, als, hybrid, hybrid_tuned, content"):
        C.baseline_names("contents")
    assert recs.check_hybrid(("model", "Content "))[0] == ("model", "content")
    assert recs.check_hybrid("content", [2.0])[:2] == (("content",), [2.0])
    with pytest.raises(ValueError, match="not one of model, popularity, itemknn, als, content"):
        recs.check_hybrid(("model", "contents"))
    with pytest.raises(ValueError, match="distinct"):
        recs.check_hybrid(("content", "content"))
    # the pinned constants are as they were
    assert recs.HYBRID_SYSTEMS == ("model", "popularity", "itemknn", "als")
    assert C.BASELINES == ("popularity", "itemknn") and C.FITTED_BASELINES == ("als",)
    assert C.FUSED_BASELINES == ("hybrid",) and C.TUNED_BASELINES == ("hybrid_tuned",)
    assert C.HYBRID_DEFAULTS == {"systems": ("model", "itemknn", "als"), "weights": None, "method": "rrf", "rrf_c": 60}
    assert list(C._systems()) == ["model", "popularity", "itemknn", "als", "content"]
    assert recs.content_batch({"n_tokens": 300}) == 4096 and recs.content_batch({"n_tokens": 300}, 7) == 7
    assert recs.content_batch({"n_tokens": 1 << 20}) == 128 and recs.content_batch({"n_tokens": 1 << 30}) == 1


# ---- host logic with ops replaced by the restatement ------------------------------------------------------------------
@pytest.fixture
def host_ops(cooc_host_ops, monkeypatch):  # noqa: F811
    """test_cooc_cpu's ``host_ops`` plus ``ops.content_scores`` as the restatement; ``content_fit`` stays on the host"""
    import torch

    def n(x):
        return None if x is None else (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))

    def content_scores(to, ti, tw, n_tokens, off, hi, hw=None, **kw):
        cooc_host_ops.append("content_scores")
        return torch.as_tensor(R.ops_content_scores(n(to), n(ti), n(tw), n_tokens, n(off), n(hi), n(hw)))

    fit = recs.content_fit
    monkeypatch.setattr(ops, "content_scores", content_scores)
    monkeypatch.setattr(recs, "content_fit", lambda meta, columns=recs.CONTENT_COLUMNS, min_df=1, max_df=1.0, device=None:
                        fit(meta, columns, min_df, max_df, device="cpu"))
    return cooc_host_ops


def _cos(fit, a, b):
    off, ti, tw = (fit[k].numpy() for k in ("tok_offsets", "tok_idx", "tok_w"))
    ra = dict(zip(ti[off[a]:off[a + 1]].tolist(), tw[off[a]:off[a + 1]].astype(np.float64)))
    return sum(ra.get(int(v), 0.0) * float(x) for v, x in zip(ti[off[b]:off[b + 1]], tw[off[b]:off[b + 1]]))


def test_content_similar_frame_host_logic(host_ops):
    df, anime_df, syn_df = _frames()
    extra = pd.DataFrame({c: ["g" if c in ("Name", "eng_version") else anime_df[c].iloc[1] for _ in range(1)]
                          for c in anime_df.columns})
    extra["anime_id"] = 70                                        # an anime nobody rated, a twin of "b" by content
    anime_df = pd.concat([anime_df, extra], ignore_index=True)
    frame, fn = C.content_similar_frame(anime_df, syn_df, "g", 4)
    assert fn == "g_content.csv" and host_ops == ["content_scores", "rows_topk"]
    assert frame.columns.tolist() == ["Name", "Similarity", "Genres", "Sypnopsis", "Episodes", "Japanese name", "Studios",
                                      "Premiered", "Score", "Type", "Source", "Rating", "Shared_tokens"]
    assert len(frame) == 4 and "g" not in frame["Name"].tolist() and frame["Name"][0] == "b"
    assert abs(frame["Similarity"][0] - 1.0) < 1e-6 and (np.diff(frame["Similarity"]) <= 0).all()
    ids = C.content_universe(anime_df)
    assert len(ids) == 7 and 70 in ids.tolist() and 70 not in set(df.anime_id)
    meta = C.metadata_by_index(ids, anime_df, syn_df)
    fit = recs.content_fit(meta)
    q = ids.tolist().index(70)
    names = meta["Name"].tolist()
    for _, r in frame.iterrows():
        j = names.index(r["Name"])
        assert abs(r["Similarity"] - _cos(fit, q, j)) < 1e-6
        toks = r["Shared_tokens"].split(" | ")
        assert 1 <= len(toks) <= C.CONTENT_SHARED_TOKENS and all("=" in t for t in toks)
        for t in toks:
            col, val = t.split("=", 1)
            assert val in C.category_tokens(meta[col][q]) and val in C.category_tokens(meta[col][j])
    assert frame["Shared_tokens"][0].split(" | ")[0] == "Type=TV" or "Genres=Action" in frame["Shared_tokens"][0]
    tv = C.content_similar_frame(anime_df, syn_df, "g", 100, types=["Movie", "OVA"])[0]
    assert set(tv["Name"]) == {"c", "e"}
    only = C.content_similar_frame(anime_df, syn_df, "a", 100, columns=["Genres"])[0]
    assert all(t.startswith("Genres=") for s in only["Shared_tokens"] if s for t in s.split(" | "))
    assert only[only["Similarity"] == 0]["Shared_tokens"].tolist() == [""] * int((only["Similarity"] == 0).sum())


def test_content_recs_frame_host_logic(host_ops):
    df, anime_df, syn_df = _frames()
    user = 1003
    mine = df[df.user_id == user]
    assert 0 < len(mine) < 6
    frame = C.content_recs_frame(df, anime_df, syn_df, user, 10, weight="centered", min_rating=0.2)
    assert host_ops == ["content_scores", "rows_topk"]
    assert frame.columns.tolist() == ["Name", "Content_score", "Genres", "Source", "anime_id", "Sypnopsis", "Episodes",
                                      "Japanese name", "Studios", "Premiered", "Score", "Type"]
    assert set(frame["anime_id"]) == set(anime_df.anime_id) - set(mine.anime_id)       # every unrated anime, no rated one
    assert (np.diff(frame["Content_score"]) <= 0).all()
    # the scores from the restatement alone
    ids = C.content_universe(anime_df)
    meta = C.metadata_by_index(ids, anime_df, syn_df)
    cols = {c: meta[c].tolist() for c in recs.CONTENT_COLUMNS}
    _, off, ti, tw = R.tfidf(cols)
    r = mine.rating.to_numpy().astype(np.float32)
    take = r >= np.float32(0.2)
    hist = [ids.tolist().index(a) for a in mine.anime_id.to_numpy()[take]]
    w = r[take] - r[take].mean(dtype=np.float32)
    want, err = R.content_scores(off, ti, tw, len(_), [0, len(hist)], hist, w)
    assert err == 0
    got = dict(zip(frame["anime_id"], frame["Content_score"]))
    assert all(np.float32(got[a]) == want[0, ids.tolist().index(a)] for a in got)
    one = C.content_recs_frame(df, anime_df, syn_df, user, 2, types=["TV"], weight="one")
    assert len(one) <= 2 and one["Type"].isin(["TV"]).all()


def test_evaluate_frame_content_host_logic(host_ops):
    table = _table()
    model = _model(table)
    rng = np.random.default_rng(9)
    genres = ["Action", "Comedy", "Drama", "Horror"]
    meta = pd.DataFrame({"Genres": [", ".join(sorted(set(rng.choice(genres, 2)))) for _ in range(table.n_anime)],
                         "Type": rng.choice(["TV", "Movie"], table.n_anime), "Source": ["Manga"] * table.n_anime,
                         "Studios": rng.choice(["A", "B", "C"], table.n_anime), "Rating": ["PG"] * table.n_anime})
    par = dict(meta=meta, columns=("Genres", "Studios"), weight="centered", min_rating=0.3)
    plain, plain_summary = C.evaluate_frame(model, table, 200, [1, 5], 0.5)
    assert "content_scores" not in host_ops
    frame, summary = C.evaluate_frame(model, table, 200, [1, 5], 0.5, baseline="content", content=par)
    assert frame.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_content", "ndcg_content"]
    assert list(summary)[-6:] == ["content_mrr", "content_mean_rank", "content_hit_rate@1", "content_ndcg@1",
                                  "content_hit_rate@5", "content_ndcg@5"]
    assert frame[["k", "hit_rate", "ndcg"]].to_csv(index=False) == plain.to_csv(index=False)
    assert {k: summary[k] for k in plain_summary} == plain_summary
    assert "content_scores" in host_ops and "rows_rank" in host_ops and "cooc_scores" not in host_ops
    # the same figures from the restatement alone, on the TRAINING slice
    users, row, anime, train = recs.held_out_targets(table, 200, 0.5)
    tu, ta, tr = table.user[train], table.anime[train], table.rating[train].astype(np.float32)
    vocab, off, ti, tw = R.tfidf({c: meta[c].tolist() for c in ("Genres", "Studios")})
    hist, hw, hoff = [], [], [0]
    for u in users:
        m = (tu == u) & (tr >= np.float32(0.3))
        hist += ta[m].tolist()
        hw += (tr[m] - tr[m].mean(dtype=np.float32)).tolist() if m.any() else []
        hoff.append(len(hist))
    scores, err = R.content_scores(off, ti, tw, len(vocab), hoff, hist, np.asarray(hw, np.float32))
    seen = np.zeros((len(users), table.n_anime), bool)
    for i, u in enumerate(users):
        seen[i, ta[tu == u]] = True
    rank, err2 = CR.rows_rank(scores, table.n_anime, table.n_anime, CR.pack_bits(seen), len(users), row, anime)
    assert err == 0 and err2 == 0
    b = recs.ranking_metrics(rank, [1, 5])
    assert summary["content_mrr"] == b["mrr"] and summary["content_mean_rank"] == b["mean_rank"]
    assert frame["hit_rate_content"].tolist() == [b["hit_rate"][1], b["hit_rate"][5]]
    assert frame["ndcg_content"].tolist() == [b["ndcg"][1], b["ndcg"][5]]
    # with others, in the documented order; as a hybrid member; with intervals
    both, both_summary = C.evaluate_frame(model, table, 200, [1, 5], 0.5, baseline=("content", "popularity"), content=par)
    assert both.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity", "hit_rate_content",
                                     "ndcg_content"]
    assert both["ndcg_content"].tolist() == frame["ndcg_content"].tolist()
    with pytest.raises(ValueError, match="rows"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="content", content=dict(par, meta=meta.iloc[:5]))
    # batches of lists change nothing
    import torch
    fit = dict(tok_offsets=torch.as_tensor(off), tok_idx=torch.as_tensor(ti), tok_w=torch.as_tensor(tw), n_tokens=len(vocab),
               n_items=table.n_anime)
    bits = CR.pack_bits(seen).view(np.int32)
    r1 = recs.content_rank(fit, hoff, hist, np.asarray(hw, np.float32), bits, row, anime, batch=3)
    np.testing.assert_array_equal(r1.numpy(), rank)
    i1, s1 = recs.content_topk(fit, hoff, hist, np.asarray(hw, np.float32), 6, bits, batch=5)
    i2, s2 = CR.rows_topk(scores, 6, wbits=CR.pack_bits(seen))
    np.testing.assert_array_equal(i1.numpy(), i2)
    assert s1.numpy().tobytes() == s2.tobytes()
    # content_similar never lists the query, and a twin scores a cosine of 1 up to the quantisation
    qi, qs = recs.content_similar(fit, [0, 3, 0], 4)
    assert qi.shape == (3, 4) and not (qi.numpy() == np.asarray([[0], [3], [0]])).any()
    assert qi.numpy()[0].tolist() == qi.numpy()[2].tolist()
    with pytest.raises(ValueError, match="out of range"):
        recs.content_similar(fit, [table.n_anime], 2)


# ---- a planted case ---------------------------------------------------------------------------------------------------
def planted():
    """two item families with disjoint token sets (items 0 .. 11 carry tokens 0 .. 5, items 12 .. 29 tokens 6 .. 14, three
    each), 16 users who rated one family alone; one own-family item of every user is held out"""
    rng = np.random.default_rng(11)
    nA, nB = 12, 18
    rows = [np.sort(rng.choice(6, 3, replace=False)) if j < nA else 6 + np.sort(rng.choice(9, 3, replace=False))
            for j in range(nA + nB)]
    x = [rng.random(3) + 0.2 for _ in rows]
    off = np.arange(nA + nB + 1, dtype=np.int64) * 3
    idx = np.concatenate(rows).astype(np.int32)
    w = np.concatenate([v / np.sqrt((v * v).sum()) for v in x]).astype(np.float32)
    hoff, hist, hw, held, seen = [0], [], [], [], np.zeros((16, nA + nB), bool)
    for u in range(16):
        fam = np.arange(nA) if u % 2 == 0 else np.arange(nA, nA + nB)
        mine = rng.choice(fam, 7, replace=False)
        held.append(int(mine[0]))
        hist += mine[1:].tolist()
        hw += (rng.integers(1, 11, 6) / 10.0).tolist()
        hoff.append(len(hist))
        seen[u, mine[1:]] = True
    return (off, idx, w, 15), (hoff, hist, np.asarray(hw, np.float32)), np.asarray(held), seen, nA


def check_planted(scores, held, seen, nA):
    for u in range(len(held)):
        own = np.arange(scores.shape[1]) < nA if u % 2 == 0 else np.arange(scores.shape[1]) >= nA
        assert (scores[u][~own] == 0).all() and not np.signbit(scores[u][~own]).any()      # disjoint tokens: exactly +0
        assert scores[u, held[u]] > 0 and own[held[u]]
        rank = int(((scores[u] > scores[u, held[u]]) & ~seen[u]).sum())
        assert rank < int((own & ~seen[u]).sum())               # above every other-family item


def test_planted_families_on_the_restatement():
    (off, idx, w, n_tokens), (hoff, hist, hw), held, seen, nA = planted()
    scores, err = R.content_scores(off, idx, w, n_tokens, hoff, hist, hw)
    assert err == 0
    check_planted(scores, held, seen, nA)
    rank, _ = CR.rows_rank(scores, 30, 30, CR.pack_bits(seen), 16, np.arange(16), held)
    assert all(rank[u] < (nA if u % 2 == 0 else 30 - nA) - 6 for u in range(16))
