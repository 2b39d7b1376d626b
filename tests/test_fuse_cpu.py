"""Hybrid lists without a GPU: the restatement against a literal per-row Python sort, the strict fall of an RRF term
with the rank, every refusal before a device is touched, the binding, the flag surface, and the host logic
(recs.hybrid_topk / hybrid_rank, components.hybrid_recs_frame, evaluate_frame(baseline="hybrid")) with ``ops`` replaced
by the restatements."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import cooc_restatement as CR
import fuse_restatement as R
from component_cli import load_component
from test_cooc_cpu import _frames, _table, host_ops  # noqa: F401  (ops as the item-kNN restatements on CPU tensors)

from anime_recommendations_amd import _lib, build, cli, components as C, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"anirec_fuse_max_items": 0, "anirec_fuse_rows": 13}
SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, 1.0, -2.5, 3e38, -3e38], np.float32)


# ---- the restatement -------------------------------------------------------------------------------------------------
def _key_literal(x):
    """the order of include/anirec.h in words: NaN last, else by value, +0 above -0"""
    if math.isnan(x):
        return (0, 0.0, 0)
    return (1, float(x), 0 if (x == 0 and math.copysign(1.0, x) < 0) else 1)


def _literal(rows, w, method, c, E):
    """the definition as Python loops over rows, systems and items"""
    nq, n = E.shape
    out = np.full((nq, n), R.NAN32, np.float32)
    f32 = np.float32
    with np.errstate(all="ignore"):
        for t in range(nq):
            el = [j for j in range(n) if E[t, j]]
            acc = {j: f32(0.0) for j in el}
            for s, r in enumerate(rows):
                x = r if r.ndim == 1 else r[t]
                order = sorted(el, key=lambda j: (tuple(-v for v in _key_literal(float(x[j]))), j))
                if method == R.RRF:
                    for place, j in enumerate(order):
                        acc[j] = f32(acc[j] + f32(f32(w[s]) / f32(c + 1 + place)))
                    continue
                fin = [j for j in order if math.isfinite(float(x[j]))]
                hi, lo = (x[fin[0]], x[fin[-1]]) if fin else (f32(0), f32(0))
                span = f32(hi - lo)
                for j in el:
                    if math.isnan(float(x[j])) or x[j] == -np.inf or (math.isfinite(float(x[j])) and span == 0):
                        v = f32(0.0)
                    elif x[j] == np.inf:
                        v = f32(1.0)
                    else:
                        v = f32(f32(x[j] - lo) / span)
                        v = R.NAN32 if np.isnan(v) else v
                    acc[j] = f32(acc[j] + f32(f32(w[s]) * v))
            for j in el:
                out[t, j] = acc[j]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("seed", range(8))
def test_restatement_equals_a_literal_python_sort(seed):
    rng = np.random.default_rng(seed)
    nq, n, S = int(rng.integers(1, 5)), int(rng.integers(1, 40)), int(rng.integers(1, 4))
    rows = []
    for s in range(S):
        x = rng.choice([rng.standard_normal((nq, n)).astype(np.float32),
                        rng.choice(SPECIAL, (nq, n)), rng.choice(np.float32([0.25, 0.5, -1, 2]), (nq, n))])
        rows.append(x[0].copy() if s == 1 else x)
    w = rng.choice(np.float32([0, 0.5, 1, 3]), S)
    w[0] = 2.0
    W = rng.random((nq, n)) < 0.3
    keep = rng.random(n) < 0.8
    for use in (False, True):
        E = R.eligible(nq, n, CR.pack_bits(W) if use else None, keep if use else None)
        assert np.array_equal(E, (~W & keep[None]) if use else np.ones((nq, n), bool))
        for method in (R.RRF, R.MINMAX):
            got = R.fuse_rows(rows, w, method, 60, n, CR.pack_bits(W) if use else None, keep if use else None, nq=nq)
            assert np.array_equal(_bits(got), _bits(_literal(rows, w, method, 60, E))), (method, use)
            assert np.array_equal(np.isnan(got) & E, np.zeros_like(E)) or method == R.MINMAX


def test_minmax_planted_row():
    x = np.float32([[2.0, 4.0, np.nan, np.inf, -np.inf, 3.0, 0.0]])
    got = R.fuse_rows([x], [2.0], R.MINMAX)
    assert got.tolist() == [[1.0, 2.0, 0.0, 2.0, 0.0, 1.5, 0.0]]
    both = np.float32([[0.0, -0.0, 0.0]])                        # hi = +0, lo = -0: a span of 0
    assert _bits(R.fuse_rows([both], None, R.MINMAX)).tolist() == [[0, 0, 0]]
    rrf = R.fuse_rows([both], None, R.RRF, 0)
    assert rrf.tolist() == [[1.0, np.float32(1 / 3), 0.5]]       # +0 above -0, ties by index
    wide = np.float32([[3e38, -3e38, 0.0]])                      # hi - lo overflows: inf / inf is the canonical NaN
    assert _bits(R.fuse_rows([wide], None, R.MINMAX)).tolist() == [[0x7FC00000, 0, 0]]


@pytest.mark.parametrize("c", (0, 1, 60, 1000, 1 << 20))
def test_an_rrf_term_falls_strictly_with_the_rank(c):
    """so one system's fused row lists the items in that system's own order: no two places share a term"""
    den = (c + 1 + np.arange(R.MAX_ITEMS, dtype=np.int64)).astype(np.float32)
    assert np.array_equal(den.astype(np.int64), c + 1 + np.arange(R.MAX_ITEMS))       # exact below 2^24
    for w in np.float32([1e-30, 1e-10, 0.1, 1.0, 7.0, 1e10, 3e38]):
        term = w / den
        assert term.dtype == np.float32 and (np.diff(term) < 0).all() and term[-1] > 0, (c, w)


# ---- the binding -----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", code))
    for name, arity in NEW.items():
        assert name in declared and len(_lib.PROTOTYPES[name][1]) == arity, name
    for text in ("#define ANIREC_FUSE_RRF     0", "#define ANIREC_FUSE_MINMAX  1", "#define ANIREC_FUSE_MAX_SYS 8"):
        assert text in code
    assert (_lib.FUSE_RRF, _lib.FUSE_MINMAX, _lib.FUSE_MAX_SYS) == (0, 1, 8) == (R.RRF, R.MINMAX, R.MAX_SYS)
    assert _lib.FUSE_METHODS == R.METHODS and _lib.FUSE_MAX_RRF_C == R.MAX_RRF_C
    assert "#define ANIREC_ABI_VERSION 5" in src and _lib.ABI_VERSION == 5
    assert "anirec_fuse.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.anirec_abi_version() == 5
    assert lib.anirec_fuse_max_items() == _lib.fuse_max_items() == R.MAX_ITEMS == 20480


def test_refusals_need_no_device():
    build.build(verbose=False)
    lib = _lib.load()
    fake = 4096

    def fuse(n_sys=2, n=10, nq=3, method=0, rrf_c=60, ld=(10, 0), w=(1.0, 0.5), ld_out=10, ptrs=None, null=()):
        S = max(len(ld), 1)
        a = dict(rows=(ctypes.c_void_p * S)(*(ptrs if ptrs is not None else [fake] * S)), ld=(ctypes.c_int64 * S)(*ld),
                 w=(ctypes.c_float * S)(*w), out=ctypes.c_void_p(fake))
        a.update({k: None for k in null})                        # a null pointer where one is required
        return lib.anirec_fuse_rows(a["rows"], a["ld"], n_sys, n, nq, None, None, a["w"], method, rrf_c, a["out"], ld_out, None)
    bad = (dict(n_sys=0), dict(n_sys=-1), dict(n_sys=9, ld=(10,) * 9, w=(1.0,) * 9), dict(n=0), dict(n=-5),
           dict(n=20481, ld=(20481, 0), ld_out=20481), dict(nq=-1), dict(ld=(9, 0)), dict(ld=(10, 5)), dict(ld=(-1, 0)),
           dict(ld_out=9), dict(method=2), dict(method=-1), dict(rrf_c=-1), dict(rrf_c=(1 << 20) + 1), dict(w=(1.0, -0.5)),
           dict(w=(float("nan"), 1.0)), dict(w=(float("inf"), 1.0)), dict(w=(0.0, 0.0)), dict(w=(-0.0, 0.0)),
           dict(ptrs=[fake, None]), dict(ptrs=[None, fake]))
    for kw in bad:
        assert fuse(**kw) == -1, kw
        if "nq" not in kw:
            assert fuse(**dict(kw, nq=0)) == -1, kw              # a bad argument is one for no rows too
    for name in ("rows", "ld", "w", "out"):
        assert fuse(null=(name,)) == -1 and fuse(null=(name,), nq=0) == -1, name
    assert fuse(nq=0) == 0                                       # no rows: nothing launched, nothing touched
    assert fuse(nq=0, n=20480, ld=(20480, 0), ld_out=20480, rrf_c=1 << 20, method=1, w=(0.0, 3e38)) == 0


def test_check_fuse_names_every_limit():
    assert ops.check_fuse(3, 17560) == (3, 17560, [1.0, 1.0, 1.0], 0, 60)
    assert ops.check_fuse(1, 20480, [0.5], " MinMax ", 1 << 20) == (1, 20480, [0.5], 1, 1 << 20)
    assert ops.check_fuse(8, 1, [0, 0, 0, 0, 0, 0, 0, 2], "RRF", 0)[3:] == (0, 0)
    for bad in (0, 9, -1, 2.5, "x", None):
        with pytest.raises(ValueError, match="1 .. 8"):
            ops.check_fuse(bad, 10)
    for bad in (0, 20481, -1, 3.5):
        with pytest.raises(ValueError, match="1 .. 20480"):
            ops.check_fuse(2, bad)
    for bad in ("borda", "", None, 3):
        with pytest.raises(ValueError, match="rrf, minmax"):
            ops.check_fuse(2, 10, None, bad)
    for bad in (-1, (1 << 20) + 1, 1.5, "x", None):
        with pytest.raises(ValueError, match="0 .. 1048576"):
            ops.check_fuse(2, 10, None, "rrf", bad)
    for bad in ([1], [1, 1, 1], []):
        with pytest.raises(ValueError, match="for 2 systems"):
            ops.check_fuse(2, 10, bad)
    for bad in ([1, -1], [float("nan"), 1], [float("inf"), 1], [1e39, 1]):
        with pytest.raises(ValueError, match=">= 0"):
            ops.check_fuse(2, 10, bad)
    with pytest.raises(ValueError, match="not all be 0"):
        ops.check_fuse(2, 10, [0, 0.0])
    with pytest.raises(ValueError, match="numbers"):
        ops.check_fuse(2, 10, ["a", "b"])


def test_system_and_weight_errors_come_before_any_gpu_use(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reached the tables")
    monkeypatch.setattr(C, "_tables_of", boom)
    monkeypatch.setattr(C, "_candidates", boom)
    assert recs.HYBRID_SYSTEMS == ("model", "popularity", "itemknn", "als")
    assert recs.check_hybrid(("Model", " als ")) == (("model", "als"), [1.0, 1.0], "rrf", 60)
    assert recs.check_hybrid("popularity", [2], "MINMAX", 0) == (("popularity",), [2.0], "minmax", 0)
    cases = ((dict(systems=("model", "knn")), "model, popularity, itemknn, als"), (dict(systems=()), "one or more"),
             (dict(systems=("als", "model", "als")), "distinct"), (dict(weights=[1, 1]), "for 3 systems"),
             (dict(weights=[1, -1, 1]), ">= 0"), (dict(weights=[0, 0, 0]), "not all be 0"), (dict(method="borda"), "rrf, minmax"),
             (dict(rrf_c=-1), "0 .. 1048576"))
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            C.hybrid_recs_frame(None, None, None, None, None, None, None, None, 7, 10, **kw)
        with pytest.raises(ValueError, match=text):
            C.evaluate_frame(None, None, 10, [1], 0.5, baseline="hybrid", hybrid=kw)
    with pytest.raises(ValueError, match="hybrid parameter"):
        C.evaluate_frame(None, None, 10, [1], 0.5, baseline="hybrid", hybrid={"k": 3})
    with pytest.raises(ValueError, match="32, 64, 128, 256"):     # a member's parameters too
        C.evaluate_frame(None, None, 10, [1], 0.5, baseline="hybrid", als={"factors": 100})
    with pytest.raises(ValueError, match="32, 64, 128, 256"):
        C.hybrid_recs_frame(None, None, None, None, None, None, None, None, 7, 10, als={"factors": 100})
    with pytest.raises(ValueError, match="itemknn parameter"):
        C.hybrid_recs_frame(None, None, None, None, None, None, None, None, 7, 10, itemknn={"k": 3})


# ---- the flag surface ------------------------------------------------------------------------------------------------
def test_baseline_names_take_hybrid_and_order_it_last():
    assert C.BASELINES == ("popularity", "itemknn") and C.FITTED_BASELINES == ("als",) and C.FUSED_BASELINES == ("hybrid",)
    assert C.baseline_names("hybrid") == ("hybrid",) and C.baseline_names(None) == ()
    assert C.baseline_names(["hybrid", "als", "popularity"]) == ("popularity", "als", "hybrid")
    assert C.baseline_names(("hybrid", "itemknn", "hybrid")) == ("itemknn", "hybrid")
    assert C.baseline_names(("als", "itemknn", "als", "popularity")) == ("popularity", "itemknn", "als")
    assert C.baseline_names("popularity") == ("popularity",) and C.baseline_names(["als"]) == ("als",)
    for wrong in ("Hybrid", "none", ["popularity", "fused"], ""):
        with pytest.raises(ValueError, match="not supported.*popularity, itemknn, als, hybrid"):
            C.baseline_names(wrong)
    assert C.HYBRID_DEFAULTS == {"systems": ("model", "itemknn", "als"), "weights": None, "method": "rrf", "rrf_c": 60}


def _argv(mod):
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    return argv


def test_hybrid_flags_in_evaluate_are_command_line_only():
    mod = load_component("evaluate")
    assert list(mod.HYBRID_FLAGS) == ["hybrid_systems", "hybrid_weights", "hybrid_method", "hybrid_rrf_c"]
    assert mod.baseline_arg("popularity, Hybrid") == ["popularity", "hybrid"]
    argv = _argv(mod)
    ns = mod.make_cli_parser().parse_args(argv)
    assert cli.hybrid_args(ns) == C.HYBRID_DEFAULTS
    ns = mod.make_cli_parser().parse_args(argv + ["--hybrid_systems", "Model, popularity", "--hybrid_weights", "[1, 0.5]",
                                                   "--hybrid_method", "MinMax", "--hybrid_rrf_c", "10"])
    assert cli.hybrid_args(ns) == {"systems": ("model", "popularity"), "weights": [1, 0.5], "method": "minmax", "rrf_c": 10}
    plain = mod.make_parser().parse_args(argv)
    assert not any(hasattr(plain, f) for f in mod.HYBRID_FLAGS)
    assert cli.hybrid_args(plain) == C.HYBRID_DEFAULTS           # a parser without the flags: the defaults
    import yaml
    params = yaml.safe_load(open(os.path.join(ROOT, "evaluate", "MLproject")))["entry_points"]["main"]["parameters"]
    assert not any(f.startswith("hybrid") for f in params)


def test_hybrid_recs_parser_and_mlproject_agree():
    mod = load_component("hybrid_recs")
    assert mod.STR_FLAGS == cli.MODEL_RECS_STR_FLAGS and mod.BOOL_FLAGS == cli.MODEL_RECS_BOOL_FLAGS
    assert mod.OPTIONAL_FLAGS == {"hybrid_systems": "model,itemknn,als", "hybrid_weights": "none", "hybrid_method": "rrf",
                                  "hybrid_rrf_c": 60}
    parser = mod.make_parser()
    argv = _argv(mod)
    ns = parser.parse_args(argv)
    assert {f: getattr(ns, f) for f in mod.OPTIONAL_FLAGS} == mod.OPTIONAL_FLAGS
    assert sorted(vars(ns)) == sorted(mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS))
    assert cli.hybrid_args(ns) == C.HYBRID_DEFAULTS
    ns = parser.parse_args(argv + ["--hybrid_systems", "als,model", "--hybrid_weights", "[2, 1]", "--hybrid_rrf_c", "0"])
    assert cli.hybrid_args(ns) == {"systems": ("als", "model"), "weights": [2, 1], "method": "rrf", "rrf_c": 0}
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "hybrid_recs", "MLproject")))
    assert ml["name"] == "hybrid_recs" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS)
    assert all(v["description"] for v in params.values())
    for f, v in params.items():
        if f in mod.OPTIONAL_FLAGS:
            assert v["default"] == mod.OPTIONAL_FLAGS[f] and v["type"] == ("int" if f == "hybrid_rrf_c" else "str")
        else:
            assert v["type"] == "str" and "default" not in v
    assert main["command"] == "python hybrid_recs.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert yaml.safe_load(open(os.path.join(ROOT, "hybrid_recs", "conda.yml")))["name"] == "hybrid_recs"


# ---- host logic with ops replaced by the restatements ----------------------------------------------------------------
def grid_of(U, A, users):
    """the stand-in for the model's ratings: the fp32 products of the rows, one add per column"""
    U, A = np.asarray(U, np.float32), np.asarray(A, np.float32)
    out = np.zeros((len(users), len(A)), np.float32)
    for c in range(U.shape[1]):
        out = (out + U[np.asarray(users, np.int64), c][:, None] * A[None, :, c]).astype(np.float32)
    return out


def als_of(n_users, n_items, seed):
    rng = np.random.default_rng(1000 + int(seed))
    return (rng.standard_normal((n_users, 8)).astype(np.float32), rng.standard_normal((n_items, 8)).astype(np.float32))


@pytest.fixture
def fuse_host_ops(host_ops, monkeypatch):  # noqa: F811
    """test_cooc_cpu's ``host_ops`` plus the fusion as its restatement, stand-ins for the model's grid and the ALS fit
    (they are not what is under test here: a fixed function of their arguments), and the model's ranks from the grid."""
    import torch

    def t(x):
        return None if x is None else torch.as_tensor(np.ascontiguousarray(x))

    def n(x):
        return None if x is None else (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))

    def fuse_rows(rows, weights=None, method="rrf", rrf_c=60, n_=None, wbits=None, keep=None):
        host_ops.append("fuse_rows")
        return t(R.ops_fuse_rows([n(r) for r in rows], weights, method, rrf_c, n_, n(wbits), n(keep)))

    def predict_grid(U, A, head, users):
        host_ops.append("predict_grid")
        return t(grid_of(n(U), n(A), n(users)))

    def predict_rank(U, A, head, users, tr, ta, watched_bits=None):
        host_ops.append("predict_rank")
        g = grid_of(n(U), n(A), n(users))
        return t(CR.ops_rows_rank(g, n(tr), n(ta), n(watched_bits))), t(g[n(tr), n(ta)])

    def predict_topk(U, A, head, users, k, watched_bits=None):
        host_ops.append("predict_topk")
        return tuple(t(x) for x in CR.ops_rows_topk(grid_of(n(U), n(A), n(users)), k, wbits=n(watched_bits)))

    def dot_scores(Q, Y, out=None):
        host_ops.append("dot_scores")
        return t(grid_of(n(Q), n(Y), np.arange(len(Q))))

    def als_fit(u, i, n_users, n_items, factors=64, sweeps=15, cg_steps=3, alpha=1.0, reg=0.01, weight=None, seed=0,
                device=None):
        host_ops.append(("als_fit", len(u), int(factors)))
        X, Y = als_of(n_users, n_items, seed)
        return {"X": t(X), "Y": t(Y)}

    for name, fn in dict(fuse_rows=fuse_rows, predict_grid=predict_grid, predict_rank=predict_rank,
                         predict_topk=predict_topk, dot_scores=dot_scores).items():
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(recs, "als_fit", als_fit)
    return host_ops


def test_hybrid_topk_and_rank_host_logic(fuse_host_ops):
    import torch
    rng = np.random.default_rng(3)
    nl, n = 7, 23
    a, b = rng.standard_normal((nl, n)).astype(np.float32), rng.choice(np.float32([0, 1, 2]), (nl, n))
    pop = rng.integers(0, 5, n).astype(np.float32)
    W = rng.random((nl, n)) < 0.3
    wb = CR.pack_bits(W).view(np.int32)
    calls = []

    def src(x):
        def f(l0, l1):
            calls.append((l0, l1))
            return torch.as_tensor(x[l0:l1])
        return f
    sources = [src(a), torch.as_tensor(pop), src(b)]
    for method, w in (("rrf", None), ("minmax", [1, 0.5, 2])):
        fused = R.fuse_rows([a, pop, b], w, R.METHODS[method], 60, n, wb)
        want = CR.rows_topk(fused, 5, wbits=wb)
        for batch in (3, 100):
            idx, sc = recs.hybrid_topk(sources, 5, w, method, 60, wb, batch=batch)
            assert np.array_equal(idx.numpy(), want[0]) and np.array_equal(_bits(sc.numpy()), _bits(want[1]))
        tr, ta = np.nonzero(~W)
        pick = rng.permutation(len(tr))[:30]
        r_want = CR.ops_rows_rank(fused, tr[pick], ta[pick], wb)
        for batch in (2, 100):
            r = recs.hybrid_rank(sources, wb, tr[pick], ta[pick], w, method, 60, batch=batch)
            assert r.dtype == torch.int32 and np.array_equal(r.numpy(), r_want)
    assert (0, 3) in calls and (6, 7) in calls and (0, 7) in calls
    keep = rng.random(n) < 0.7
    idx, _ = recs.hybrid_topk(sources, n, None, "rrf", 60, wb, keep.astype(np.uint8))
    assert all(set(i[i >= 0].tolist()) == set(np.flatnonzero(~W[t] & keep).tolist()) for t, i in enumerate(idx.numpy()))
    st, sa = np.nonzero(W)
    with pytest.raises(ValueError, match="own watched bit"):
        recs.hybrid_rank(sources, wb, [int(st[0])], [int(sa[0])])
    with pytest.raises(ValueError, match="target_row out of range"):
        recs.hybrid_rank(sources, wb, [nl], [0])
    with pytest.raises(ValueError, match="n_lists"):
        recs.hybrid_topk(sources, 3)
    assert recs.hybrid_rank(sources, wb, [], []).numel() == 0
    one = recs.hybrid_rank([src(a)], wb, tr[pick], ta[pick])     # one system: that system's own ranks
    assert np.array_equal(one.numpy(), CR.ops_rows_rank(a, tr[pick], ta[pick], wb))


def _model_of(n_users, n_anime, seed=2):
    rng = np.random.default_rng(seed)
    head = dict(w=1.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0)
    return (rng.standard_normal((n_users, 4)).astype(np.float32), rng.standard_normal((n_anime, 4)).astype(np.float32), head)


def expected_hybrid_frame(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs, grid, als_rows, types=None,
                          genres=None, systems=("model", "itemknn", "als"), weights=None, method="rrf", rrf_c=60,
                          itemknn=None, als=None):
    """``hybrid_recs_frame`` from the restatements alone: ``grid(users)`` the model's rows, ``als_rows(ui, ai, par, row)`` the
    ALS member's.  Returns (frame, stats)."""
    knn_par = dict(C.ITEMKNN_DEFAULTS, **(itemknn or {}))
    als_par = dict(C.ALS_DEFAULTS, **(als or {}))
    row = int(np.nonzero(np.asarray(user_ids) == int(user_id))[0][0])
    meta = C.metadata_by_index(anime_ids, anime_df, syn_df)
    blocked = ~C.filter_mask(meta, anime_df, types, genres) | ~C.unwatched_mask(df, anime_ids, user_id)
    wb = CR.pack_bits(blocked[None])
    ui, ai, r = C.rating_indices(df, user_ids, anime_ids)
    n_users, n_anime = len(user_ids), len(anime_ids)
    rows = {"model": grid([row])}
    if "popularity" in systems:
        rows["popularity"] = np.bincount(ai, minlength=n_anime).astype(np.float32)[None]
    if "itemknn" in systems:
        liked = r.astype(np.float32) >= np.float32(knn_par["min_rating"])
        L = np.zeros((n_anime, n_users), bool)
        L[ai[liked], ui[liked]] = True
        sim, _, excl, _, _ = CR.cooc_scores(CR.pack_bits(L), n_users, np.arange(n_anime), CR.MEASURES[knn_par["measure"]],
                                            knn_par["shrink"], knn_par["min_support"])
        ni, ns = CR.rows_topk(sim, int(knn_par["neighbours"]), wbits=excl)
        hist = ai[(ui == row) & liked]
        rows["itemknn"], err = CR.itemknn_scores(ni, ns, [0, len(hist)], hist)
        assert err == 0
    if "als" in systems:
        liked = r.astype(np.float32) >= np.float32(als_par["min_rating"])
        rows["als"] = als_rows(ui[liked], ai[liked], als_par, row)
    w = [1.0] * len(systems) if weights is None else weights
    fused = R.fuse_rows([rows[s] for s in systems], w, R.METHODS[method], rrf_c, n_anime, wb)
    k = min(int(n_recs), n_anime)
    idx, sc = CR.rows_topk(fused, k, wbits=wb)
    idx, sc = idx[0], sc[0]
    ok = idx >= 0
    frame = C._model_recs_rows(meta, idx, np.where(ok, rows["model"][0][np.maximum(idx, 0)], np.float32(np.nan)))
    frame["Hybrid_score"] = sc[ok]
    for s in systems:
        frame["Rank_" + s] = CR.ops_rows_rank(rows[s], np.zeros(int(ok.sum()), np.int64), idx[ok], wb).astype(np.int64) + 1
    return frame, {"hybrid_systems": list(systems), "hybrid_weights": [float(x) for x in w], "hybrid_method": method,
                   "hybrid_rrf_c": int(rrf_c)}


def test_hybrid_recs_frame_host_logic(fuse_host_ops):
    df, anime_df, syn_df = _frames()
    user_ids, anime_ids = C.index_tables({}, df)
    U, A, head = _model_of(len(user_ids), len(anime_ids))
    user = int(df.user_id.value_counts().index[-1])              # a user with few ratings: candidates are left
    tables = (U, A, head, user_ids, anime_ids, df, anime_df, syn_df)

    def als_rows(ui, ai, par, row):
        X, Y = als_of(len(user_ids), len(anime_ids), par["seed"])
        return grid_of(X[[row]], Y, [0])
    for kw in (dict(), dict(systems=("popularity", "model"), weights=[2, 1], method="minmax"),
               dict(systems=("als", "itemknn"), rrf_c=0, itemknn=dict(neighbours=3, min_rating=0.4), als=dict(seed=5)),
               dict(types=["TV"]), dict(systems=("model",))):
        frame, stats = C.hybrid_recs_frame(*tables, user, 4, **kw)
        want, want_stats = expected_hybrid_frame(*tables, user, 4, lambda us: grid_of(U, A, us), als_rows, **kw)
        assert frame.to_csv(index=False) == want.to_csv(index=False) and stats == want_stats, kw
        members = stats["hybrid_systems"]
        assert frame.columns.tolist() == ["Name", "Prediction", "Genres", "Source", "anime_id", "Sypnopsis", "Episodes",
                                          "Japanese name", "Studios", "Premiered", "Score", "Type", "Hybrid_score"] + \
            ["Rank_" + m for m in members]
        assert 0 < len(frame) <= 4 and (np.diff(frame["Hybrid_score"]) <= 0).all()
        assert not set(frame["anime_id"]) & set(df[df.user_id == user].anime_id)
    assert set(C.hybrid_recs_frame(*tables, user, 6, types=["TV"])[0]["Type"]) == {"TV"}
    solo = C.hybrid_recs_frame(*tables, user, 6, systems=("model",))[0]
    assert solo["Rank_model"].tolist() == list(range(1, len(solo) + 1))
    plain = C.model_recs_frame(*tables, user, 6)                 # one member: that member's own list
    assert solo["anime_id"].tolist() == plain["anime_id"].tolist()
    assert solo["Prediction"].tolist() == plain["Prediction"].tolist()
    with pytest.raises(ValueError, match="no embedding row"):
        C.hybrid_recs_frame(*tables, -5, 4)


def test_evaluate_frame_hybrid_host_logic(fuse_host_ops):
    table = _table()
    U, A, head = _model_of(table.n_users, table.n_anime)
    model = dict(U=U, A=A, head=head, user_ids=table.user_ids, anime_ids=table.anime_ids)
    ks = [1, 5]
    plain, plain_summary = C.evaluate_frame(model, table, 200, ks, 0.5)
    same, same_summary = C.evaluate_frame(model, table, 200, ks, 0.5, hybrid={"systems": ("model", "popularity")})
    assert "fuse_rows" not in fuse_host_ops                      # without the baseline nothing of it runs
    assert same.to_csv(index=False) == plain.to_csv(index=False) and same_summary == plain_summary
    par = dict(neighbours=4, measure="jaccard", shrink=0.5, min_support=2, min_rating=0.4)
    hyb = dict(systems=("model", "popularity", "itemknn", "als"), weights=[1, 0.5, 2, 1], method="rrf", rrf_c=10)
    frame, summary = C.evaluate_frame(model, table, 200, ks, 0.5, baseline=("hybrid", "popularity"), itemknn=par,
                                      als={"seed": 3}, hybrid=hyb, ci_replicates=0)
    assert frame.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity", "hit_rate_hybrid",
                                      "ndcg_hybrid"]
    assert list(summary)[:len(plain_summary)] == list(plain_summary)
    assert list(summary)[-6:] == ["hybrid_mrr", "hybrid_mean_rank", "hybrid_hit_rate@1", "hybrid_ndcg@1", "hybrid_hit_rate@5",
                                  "hybrid_ndcg@5"]
    assert frame[["k", "hit_rate", "ndcg"]].to_csv(index=False) == plain.to_csv(index=False)
    assert sum(1 for c in fuse_host_ops if isinstance(c, tuple) and c[0] == "als_fit") == 1
    # the same figures from the restatements alone, every member fitted on the TRAINING slice
    users, row, anime, train = recs.held_out_targets(table, 200, 0.5)
    tu, ta, tr = table.user[train], table.anime[train], table.rating[train].astype(np.float32)
    liked = tr >= np.float32(0.4)
    L = np.zeros((table.n_anime, table.n_users), bool)
    L[ta[liked], tu[liked]] = True
    sim, _, excl, _, _ = CR.cooc_scores(CR.pack_bits(L), table.n_users, np.arange(table.n_anime), CR.JACCARD, 0.5, 2)
    ni, ns = CR.rows_topk(sim, 4, wbits=excl)
    off = np.concatenate([[0], np.cumsum([int(((tu == u) & liked).sum()) for u in users])])
    hist = np.concatenate([ta[(tu == u) & liked] for u in users])
    knn_rows, err = CR.itemknn_scores(ni, ns, off, hist)
    assert err == 0
    seen = np.zeros((len(users), table.n_anime), bool)
    for i, u in enumerate(users):
        seen[i, ta[tu == u]] = True
    wb = CR.pack_bits(seen)
    X, Y = als_of(table.n_users, table.n_anime, 3)
    rows = [grid_of(U, A, users), np.bincount(ta, minlength=table.n_anime).astype(np.float32), knn_rows,
            grid_of(X[users], Y, np.arange(len(users)))]
    fused = R.fuse_rows(rows, hyb["weights"], R.RRF, 10, table.n_anime, wb)
    rank = CR.ops_rows_rank(fused, row, anime, wb)
    b = recs.ranking_metrics(rank, ks)
    assert summary["hybrid_mrr"] == b["mrr"] and summary["hybrid_mean_rank"] == b["mean_rank"]
    assert frame["hit_rate_hybrid"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_hybrid"].tolist() == [b["ndcg"][k] for k in ks]
    # a fit is shared with the baseline of the same name; the order of the systems is the library's
    fuse_host_ops.clear()
    both, both_summary = C.evaluate_frame(model, table, 200, ks, 0.5, baseline=("hybrid", "als", "itemknn"), itemknn=par,
                                          als={"seed": 3}, hybrid=hyb)
    assert both.columns.tolist()[3:] == ["hit_rate_itemknn", "ndcg_itemknn", "hit_rate_als", "ndcg_als", "hit_rate_hybrid",
                                         "ndcg_hybrid"]
    assert sum(1 for c in fuse_host_ops if isinstance(c, tuple) and c[0] == "als_fit") == 1
    assert both["ndcg_hybrid"].tolist() == frame["ndcg_hybrid"].tolist() and both_summary["hybrid_mrr"] == summary["hybrid_mrr"]
    solo = C.evaluate_frame(model, table, 200, ks, 0.5, baseline="hybrid", hybrid={"systems": ("model",)})[0]
    assert solo["hit_rate_hybrid"].tolist() == solo["hit_rate"].tolist()      # one member: the member's own ranks
    assert solo["ndcg_hybrid"].tolist() == solo["ndcg"].tolist()


def test_hybrid_frames_on_the_recs_fixture(fuse_host_ops, tmp_path):
    """the two frames on the recs fixture (14 users x 560 anime), every op a restatement or a stand-in"""
    import recs_fixture as RF
    from anime_recommendations_amd import data
    rec = RF.load()
    z, df = rec["npz"], RF.ratings(rec)
    anime_df, syn_df = C.load_anime_df(RF.csv(rec, "anime_csv")), C.load_synopses(RF.csv(rec, "synopses_csv"))
    user_ids, anime_ids = C.index_tables({}, df)
    U, A = np.asarray(z["U"], np.float32), np.asarray(z["A"], np.float32)
    head = dict(rec["model_recs"]["heads"]["sigmoid"], activation="sigmoid")
    tables = (U, A, head, user_ids, anime_ids, df, anime_df, syn_df)
    user = int(rec["model_recs"]["cases"][0]["user"])

    def als_rows(ui, ai, par, row):
        X, Y = als_of(len(user_ids), len(anime_ids), par["seed"])
        return grid_of(X[[row]], Y, [0])
    kw = dict(types=C.literal(rec["flags"]["MR_TYPES"]), weights=[1, 0.5, 2], rrf_c=10, itemknn=dict(neighbours=20, min_rating=0.6))
    frame, stats = C.hybrid_recs_frame(*tables, user, 15, **kw)
    want, want_stats = expected_hybrid_frame(*tables, user, 15, lambda us: grid_of(U, A, us), als_rows, **kw)
    assert frame.to_csv(index=False) == want.to_csv(index=False) and stats == want_stats
    assert len(frame) == 15 and frame["Type"].isin(kw["types"]).all() and (np.diff(frame["Hybrid_score"]) <= 0).all()
    # evaluate on the same ratings: the hybrid of the model and popularity from the restatement alone
    pq = str(tmp_path / "user_stats.parquet")
    df.to_parquet(pq, index=False)
    table = data.load_user_stats(pq)
    model = dict(U=U, A=A, head=head, user_ids=table.user_ids, anime_ids=table.anime_ids)
    ks, hyb = [1, 5, 20], dict(systems=("popularity", "model"), method="minmax", weights=[0.5, 1])
    plain, plain_summary = C.evaluate_frame(model, table, 1000, ks, 0.7)
    got, summary = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline="hybrid", hybrid=hyb)
    assert got[["k", "hit_rate", "ndcg"]].to_csv(index=False) == plain.to_csv(index=False)
    assert {k: summary[k] for k in plain_summary} == plain_summary
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    assert len(row) > 100
    tu, ta = np.asarray(table.user[train]), np.asarray(table.anime[train])
    seen = np.zeros((len(users), table.n_anime), bool)
    for i, u in enumerate(users):
        seen[i, ta[tu == u]] = True
    wb = CR.pack_bits(seen)
    fused = R.fuse_rows([np.bincount(ta, minlength=table.n_anime).astype(np.float32), grid_of(U, A, users)], [0.5, 1], R.MINMAX,
                        60, table.n_anime, wb)
    b = recs.ranking_metrics(CR.ops_rows_rank(fused, row, anime, wb), ks)
    assert got["hit_rate_hybrid"].tolist() == [b["hit_rate"][k] for k in ks]
    assert got["ndcg_hybrid"].tolist() == [b["ndcg"][k] for k in ks] and summary["hybrid_mrr"] == b["mrr"]
