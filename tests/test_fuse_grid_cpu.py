"""Learned hybrid weights without a GPU: the restatement of the rank grid against plain Python loops,
the grid generator, every refusal that needs no device, the tie rule of the fit, the flag surface of evaluate, and
evaluate_frame's host logic with ``ops`` replaced by the restatements.  Every comparison is an integer equality."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import boot_restatement as BR
import cooc_restatement as CR
import fuse_grid_restatement as G
import fuse_restatement as R
from component_cli import load_component
from test_cooc_cpu import _table, host_ops  # noqa: F401  (ops as the item-kNN restatements on CPU tensors)
from test_fuse_cpu import SPECIAL, _argv, _key_literal, _literal, _model_of, als_of, fuse_host_ops, grid_of  # noqa: F401

from anime_recommendations_amd import _lib, build, components as C, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"anirec_fuse_rank_grid_workspace_bytes": 4, "anirec_fuse_rank_grid": 19}


# ---- the restatement -------------------------------------------------------------------------------------------------
def _rank_literal(fused_row, e, a):
    """the place of item ``a`` in the literal order of the eligible items: larger first, +0 above -0, NaN last, ties by
    the index"""
    order = sorted([j for j in range(len(e)) if e[j]],
                   key=lambda j: (tuple(-v for v in _key_literal(float(fused_row[j]))), j))
    return order.index(a)


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_plain_python_loops(seed):
    rng = np.random.default_rng(seed)
    nq, n, S = int(rng.integers(1, 4)), int(rng.integers(1, 24)), int(rng.integers(1, 4))
    rows = []
    for s in range(S):
        x = rng.choice([rng.standard_normal((nq, n)).astype(np.float32), rng.choice(SPECIAL, (nq, n)),
                        rng.choice(np.float32([0.25, 0.5, -1, 2]), (nq, n))])
        rows.append(x[0].copy() if s == 1 else x)
    grid = rng.choice(np.float32([0, 0.5, 1, 3]), (4, S))
    grid[:, 0] = 2.0
    W = rng.random((nq, n)) < 0.3
    keep = rng.random(n) < 0.8
    for use in (False, True):
        wb, kp = (CR.pack_bits(W), keep) if use else (None, None)
        E = R.eligible(nq, n, wb, kp)
        tr, ta = np.nonzero(E)
        for method in (R.RRF, R.MINMAX):
            got, err = G.rank_grid(rows, grid, method, 60, tr, ta, n, wb, kp, nq=nq)
            assert err == 0 and got.shape == (4, len(tr)) and got.dtype == np.int32
            for w in range(4):
                fused = _literal(rows, grid[w], method, 60, E)
                want = [_rank_literal(fused[r], E[r], a) for r, a in zip(tr, ta)]
                assert got[w].tolist() == want, (method, use, w)


def test_restatement_marks_bad_targets_and_bad_weight_vectors():
    rng = np.random.default_rng(1)
    rows = [rng.standard_normal((2, 9)).astype(np.float32), rng.standard_normal(9).astype(np.float32)]
    W = np.zeros((2, 9), bool)
    W[1, 4] = True
    keep = np.ones(9, np.uint8)
    keep[7] = 0
    grid = np.float32([[1, 1], [1, -1], [0, 0], [np.nan, 1], [np.inf, 1], [0, 2]])
    tr, ta = [0, 1, 2, -1, 0, 0, 1, 0], [3, 4, 0, 0, 9, -1, 3, 7]
    got, err = G.rank_grid(rows, grid, R.RRF, 60, tr, ta, 9, CR.pack_bits(W), keep)
    assert err == 1
    assert (got[1:5] == -1).all()                                # the bad vectors: their whole rows
    for w in (0, 5):
        assert (got[w][[1, 2, 3, 4, 5, 7]] == -1).all() and (got[w][[0, 6]] >= 0).all()
    clean, err = G.rank_grid(rows, grid[[0, 5]], R.RRF, 60, [0, 1], [3, 3], 9, CR.pack_bits(W), keep)
    assert err == 0 and np.array_equal(clean, got[[0, 5]][:, [0, 6]])    # the others are unaffected


# ---- the grid generator ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sys, steps", [(1, 1), (1, 7), (2, 1), (2, 10), (3, 10), (3, 4), (4, 5), (8, 2), (5, 3)])
def test_weight_grid_rows_and_order(n_sys, steps):
    g = recs.hybrid_weight_grid(n_sys, steps)
    assert g.dtype == np.float32 and g.shape == (1 + math.comb(steps + n_sys - 1, n_sys - 1), n_sys)
    assert (g[0] == 1).all()
    assert np.array_equal(g.view(np.uint32), G.weight_grid(n_sys, steps).view(np.uint32))
    ints = np.rint(g[1:].astype(np.float64) * steps).astype(np.int64)
    assert (ints.sum(axis=1) == steps).all() and (ints >= 0).all()
    assert [tuple(r) for r in ints] == sorted(set(tuple(r) for r in ints))      # ascending, none twice
    assert np.array_equal(g[1:], (ints / np.float64(steps)).astype(np.float32))
    ops.check_fuse_grid(n_sys, 10, g)                            # every vector is one the kernel takes


def test_weight_grid_limits():
    assert len(recs.hybrid_weight_grid(3, 10)) == 67
    assert len(recs.hybrid_weight_grid(3, 88)) == 4006 and len(recs.hybrid_weight_grid(2, 4093)) == 4095
    for n_sys, steps in ((3, 89), (2, 4094), (8, 8), (4, 28)):
        with pytest.raises(ValueError, match="4095"):
            recs.hybrid_weight_grid(n_sys, steps)
    for steps in (0, -3):
        with pytest.raises(ValueError, match=">= 1"):
            recs.hybrid_weight_grid(3, steps)
    for n_sys in (0, 9):
        with pytest.raises(ValueError, match="1 .. 8"):
            recs.hybrid_weight_grid(n_sys, 2)
    assert ops.FUSE_MAX_GRID == _lib.FUSE_MAX_GRID == G.MAX_GRID == 4095 == ops.BOOT_MAX_COL - 1


# ---- the binding and the refusals ------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", code))
    for name, arity in NEW.items():
        assert name in declared and len(_lib.PROTOTYPES[name][1]) == arity, name
    assert "#define ANIREC_FUSE_MAX_GRID 4095" in code
    assert "#define ANIREC_ABI_VERSION 5" in src and _lib.ABI_VERSION == 5      # additive: the ABI stays
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    assert _lib.PROTOTYPES["anirec_fuse_rank_grid_workspace_bytes"] == (sz, [i32] * 4)
    assert _lib.PROTOTYPES["anirec_fuse_rank_grid"] == (ctypes.c_int, [
        ctypes.POINTER(vp), ctypes.POINTER(i64), i32, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, sz, vp])
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    size = lib.anirec_fuse_rank_grid_workspace_bytes
    assert size(3, 17560, 10, 0) == size(3, 17560, 10, 1) == 10 * 3 * 17560 * 4
    assert size(1, 1, 1, 0) == 16 and size(2, 5, 3, 1) == 3 * 2 * 8 * 4 and size(3, 10, 0, 0) == 0
    for bad in ((0, 10, 1, 0), (9, 10, 1, 0), (1, 0, 1, 0), (1, 20481, 1, 0), (1, 10, -1, 0), (1, 10, 1, 2), (1, 10, 1, -1)):
        assert size(*bad) == 0, bad


def test_refusals_need_no_device():
    build.build(verbose=False)
    lib = _lib.load()
    fake = 4096

    def grid(n_sys=2, n=10, n_rows=3, method=0, rrf_c=60, ld=(10, 0), n_w=5, n_t=4, ptrs=None, null=(), ws_bytes=1 << 20,
             ws=fake):
        S = max(len(ld), 1)
        a = dict(rows=(ctypes.c_void_p * S)(*(ptrs if ptrs is not None else [fake] * S)), ld=(ctypes.c_int64 * S)(*ld),
                 weights=ctypes.c_void_p(fake), tr=ctypes.c_void_p(fake), ta=ctypes.c_void_p(fake),
                 out=ctypes.c_void_p(fake), err=ctypes.c_void_p(fake))
        a.update({k: None for k in null})
        return lib.anirec_fuse_rank_grid(a["rows"], a["ld"], n_sys, n, n_rows, None, None, method, rrf_c, a["weights"], n_w,
                                         a["tr"], a["ta"], n_t, a["out"], a["err"], ws, ws_bytes, None)
    bad = (dict(n_sys=0), dict(n_sys=-1), dict(n_sys=9, ld=(10,) * 9), dict(n=0), dict(n=-5), dict(n=20481, ld=(20481, 0)),
           dict(n_rows=-1), dict(ld=(9, 0)), dict(ld=(10, 5)), dict(ld=(-1, 0)), dict(method=2), dict(method=-1),
           dict(rrf_c=-1), dict(rrf_c=(1 << 20) + 1), dict(ptrs=[fake, None]), dict(ptrs=[None, fake]),
           dict(n_w=0), dict(n_w=-1), dict(n_w=4096), dict(n_t=-1))
    for kw in bad:
        assert grid(**kw) == -1, kw
        if "n_t" not in kw:
            assert grid(**dict(kw, n_t=0)) == -1, kw             # a bad argument is one for no targets too
        if "n_rows" not in kw:
            assert grid(**dict(kw, n_rows=0)) == -1, kw
    for name in ("rows", "ld", "weights", "out", "err"):
        assert grid(null=(name,)) == -1 and grid(null=(name,), n_t=0) == -1, name
    for name in ("tr", "ta"):
        assert grid(null=(name,)) == -1 and grid(null=(name,), n_t=0) == 0, name     # no targets: no target arrays
    assert grid(n_t=0) == 0 and grid(n_rows=0) == 0 and grid(n_t=0, n_w=4095) == 0   # nothing launched, nothing touched
    need = 3 * 2 * 12 * 4
    assert lib.anirec_status_string(grid(ws_bytes=need - 1)).decode() == lib.anirec_status_string(
        grid(ws_bytes=0, ws=None)).decode() != lib.anirec_status_string(-1).decode()     # ANIREC_EWORKSPACE
    assert grid(ws_bytes=need - 1) != 0 and grid(ws_bytes=need, ws=None) == -1 and grid(ws_bytes=need, ws=fake + 4) == -1


def test_check_fuse_grid_names_every_limit():
    si, ni, g, m, c = ops.check_fuse_grid(3, 17560, [[1, 1, 1], [0, 0.5, 0.5]], " MinMax ", 7)
    assert (si, ni, m, c) == (3, 17560, 1, 7) and g.dtype == np.float32 and g.shape == (2, 3) and g.flags.c_contiguous
    assert ops.check_fuse_grid(1, 20480, np.ones((4095, 1)))[2].shape == (4095, 1)
    import torch
    assert ops.check_fuse_grid(2, 5, torch.ones(3, 2))[2].tolist() == [[1, 1]] * 3
    # everything check_fuse refuses
    for bad in (0, 9, -1, 2.5, "x", None):
        with pytest.raises(ValueError, match="1 .. 8"):
            ops.check_fuse_grid(bad, 10, [[1]])
    for bad in (0, 20481, -1, 3.5):
        with pytest.raises(ValueError, match="1 .. 20480"):
            ops.check_fuse_grid(2, bad, [[1, 1]])
    for bad in ("borda", "", None, 3):
        with pytest.raises(ValueError, match="rrf, minmax"):
            ops.check_fuse_grid(2, 10, [[1, 1]], bad)
    for bad in (-1, (1 << 20) + 1, 1.5, "x", None):
        with pytest.raises(ValueError, match="0 .. 1048576"):
            ops.check_fuse_grid(2, 10, [[1, 1]], "rrf", bad)
    # the grid's shape and size
    for bad in ([1, 1], [[1], [1]], [[1, 1, 1]], np.ones((0, 2)), np.ones((4096, 2)), np.ones((2, 2, 2)), 1.0):
        with pytest.raises(ValueError, match=r"n_sys = 2.*1 \.\. 4095"):
            ops.check_fuse_grid(2, 10, bad)
    with pytest.raises(ValueError, match="numbers"):
        ops.check_fuse_grid(2, 10, [["a", "b"]])
    # any bad weight vector, named by its index
    for bad in ([1, -1], [float("nan"), 1], [float("inf"), 1], [1e39, 1], [0, 0], [-0.0, 0.0]):
        with pytest.raises(ValueError, match="weight vector 2 .*>= 0 and not all 0"):
            ops.check_fuse_grid(2, 10, [[1, 1], [0, 1], bad, [1, 0]])


def test_wrapper_refusals_come_before_the_device(monkeypatch):
    import torch
    monkeypatch.setattr(ops, "_need_gpu", lambda: (_ for _ in ()).throw(AssertionError("reached the device")))
    x = torch.zeros(2, 10)
    with pytest.raises(ValueError, match="1 .. 4095"):
        ops.fuse_rank_grid([x, x], np.ones((4096, 2)), "rrf", 60, [0], [0])
    with pytest.raises(ValueError, match="weight vector 0"):
        ops.fuse_rank_grid([x, x], [[1, -1]], "rrf", 60, [0], [0])
    with pytest.raises(ValueError, match="shortest row"):
        ops.fuse_rank_grid([x], [[1]], "rrf", 60, [0], [0], n=11)
    with pytest.raises(ValueError, match="device tensor"):
        ops.fuse_rank_grid([x, 3.0], [[1, 1]], "rrf", 60, [0], [0])
    wb = torch.zeros(2, 1, dtype=torch.int32)
    for kw, text in ((dict(weight_grid=np.ones((4096, 1))), "1 .. 4095"), (dict(weight_grid=[[0.0]]), "weight vector 0"),
                     (dict(method="borda"), "rrf, minmax"), (dict(batch=0), "batch must be >= 1"),
                     (dict(target_row=[2]), "target_row out of range")):
        args = dict(dict(weight_grid=[[1.0]], method="rrf", batch=4, target_row=[0]), **kw)
        with pytest.raises(ValueError, match=text):
            recs.hybrid_rank_grid([lambda l0, l1: x[l0:l1]], wb, args["target_row"], [0], args["weight_grid"],
                                  args["method"], 60, args["batch"])
    with pytest.raises(ValueError, match="watched_bits"):
        recs.hybrid_rank_grid([x], None, [0], [0], [[1.0]])


# ---- the fit ---------------------------------------------------------------------------------------------------------
def test_tune_metric_names():
    assert recs.hybrid_tune_metric(" NDCG@10 ") == ("ndcg@10", 10) and recs.hybrid_tune_metric("mrr") == ("mrr", None)
    assert recs.hybrid_tune_metric("hit_rate@1") == ("hit_rate@1", 1)
    for bad in ("ndcg", "ndcg@0", "ndcg@-1", "ndcg@x", "mean_rank", "hit@5", "", None, "mrr@3"):
        with pytest.raises(ValueError, match="ndcg@K, hit_rate@K, mrr"):
            recs.hybrid_tune_metric(bad)


def test_best_weights_ties_go_to_the_lowest_index():
    sums = np.array([[5, 9, 9, 2], [4, 0, 0, 7]], np.int64)      # totals 9, 9, 9, 9
    assert recs.hybrid_best_weights(sums) == 0 == G.best(sums, [True, True])
    assert recs.hybrid_best_weights(sums, [0]) == 1 == G.best(sums, [True, False])      # 9 twice: the first of them
    assert recs.hybrid_best_weights(sums, np.array([False, True])) == 3
    sums[1, 2] = 1                                               # now vector 2 is strictly better
    assert recs.hybrid_best_weights(sums) == 2 == G.best(sums, [True, True])
    big = np.array([[1 << 61, (1 << 61) + 1]], np.int64)         # an exact integer sum, not a float one
    assert recs.hybrid_best_weights(big) == 1
    assert recs.hybrid_cross_fit(sums, [0, 1], 2) == [3, 1] == G.cross_fit(sums, [0, 1], 2)


@pytest.mark.parametrize("metric", ("ndcg@3", "hit_rate@2", "mrr"))
def test_fit_weights_host_logic(monkeypatch, metric):
    import torch
    monkeypatch.setattr(ops, "rank_gain_rows", BR.ops_rank_gain_rows)
    rng = np.random.default_rng(4)
    n_w, n_t, n_units, n_rows = 6, 40, 7, 12
    ranks = rng.integers(-1, n_rows + 2, (n_w, n_t)).astype(np.int32)      # -1 and ranks past the table gain nothing
    ranks[3] = ranks[1]                                          # two vectors with equal sums
    unit = rng.integers(0, n_units, n_t)
    sums, best = recs.hybrid_fit_weights(torch.as_tensor(ranks), unit, n_units, metric, n_rows)
    want = G.gain_sums(ranks, unit, n_units, metric, n_rows)
    assert sums.dtype == np.int64 and np.array_equal(sums, want) and np.array_equal(sums[:, 1], sums[:, 3])
    assert best == G.best(want, np.ones(n_units, bool))
    mask = rng.random(n_units) < 0.5
    assert recs.hybrid_fit_weights(torch.as_tensor(ranks), unit, n_units, metric, n_rows, mask)[1] == G.best(want, mask)
    ranks[1] = 0                                                 # both the best now: the lower index wins
    ranks[3] = 0
    assert recs.hybrid_fit_weights(torch.as_tensor(ranks), unit, n_units, metric, n_rows)[1] == 1


def test_fold_deal_and_cross_fit():
    for n, folds, seed in ((10, 2, 0), (11, 3, 5), (3, 5, 1), (0, 2, 0)):
        fold = recs.hybrid_fold_deal(n, folds, seed)
        assert fold.dtype == np.int64 and np.array_equal(fold, G.fold_deal(n, folds, seed))
        assert np.array_equal(np.bincount(fold, minlength=folds)[:folds],
                              np.bincount(np.arange(n) % folds, minlength=folds))      # dealt evenly
    for bad in (1, 0, -2):
        with pytest.raises(ValueError, match="folds >= 2"):
            recs.hybrid_fold_deal(10, bad, 0)
    rng = np.random.default_rng(2)
    sums = rng.integers(0, 1000, (9, 5))
    fold = recs.hybrid_fold_deal(9, 3, 4)
    picks = recs.hybrid_cross_fit(sums, fold, 3)
    assert picks == G.cross_fit(sums, fold, 3)
    for f in range(3):                                           # a fold's choice never depends on that fold's own sums
        other = sums.copy()
        other[fold == f] = rng.integers(0, 10 ** 6, (int((fold == f).sum()), 5))
        assert recs.hybrid_cross_fit(other, fold, 3)[f] == picks[f]


# ---- the flag surface ------------------------------------------------------------------------------------------------
def test_baseline_names_take_hybrid_tuned_last():
    assert C.TUNED_BASELINES == ("hybrid_tuned",) and C.FUSED_BASELINES == ("hybrid",)
    assert C.baseline_names("hybrid_tuned") == ("hybrid_tuned",)
    assert C.baseline_names(["hybrid_tuned", "als", "hybrid", "popularity"]) == ("popularity", "als", "hybrid", "hybrid_tuned")
    with pytest.raises(ValueError, match="not supported.*popularity, itemknn, als, hybrid, hybrid_tuned"):
        C.baseline_names("tuned")
    assert C.HYBRID_TUNE_DEFAULTS == {"metric": "ndcg@10", "steps": 10, "folds": 2, "seed": 0}


def test_tune_flags_in_evaluate_are_command_line_only():
    mod = load_component("evaluate")
    assert {f: v[1] for f, v in mod.HYBRID_TUNE_FLAGS.items()} == {"hybrid_tune_" + k: v
                                                                    for k, v in C.HYBRID_TUNE_DEFAULTS.items()}
    assert mod.baseline_arg("hybrid, Hybrid_Tuned") == ["hybrid", "hybrid_tuned"]
    argv = _argv(mod)
    ns = mod.make_cli_parser().parse_args(argv)
    assert {f: getattr(ns, f) for f in mod.HYBRID_TUNE_FLAGS} == {f: v[1] for f, v in mod.HYBRID_TUNE_FLAGS.items()}
    ns = mod.make_cli_parser().parse_args(argv + ["--hybrid_tune_metric", "mrr", "--hybrid_tune_steps", "4",
                                                   "--hybrid_tune_folds", "5", "--hybrid_tune_seed", "9"])
    assert (ns.hybrid_tune_metric, ns.hybrid_tune_steps, ns.hybrid_tune_folds, ns.hybrid_tune_seed) == ("mrr", 4, 5, 9)
    plain = mod.make_parser().parse_args(argv)
    assert not any(hasattr(plain, f) for f in mod.HYBRID_TUNE_FLAGS)
    import yaml
    params = yaml.safe_load(open(os.path.join(ROOT, "evaluate", "MLproject")))["entry_points"]["main"]["parameters"]
    assert not any(f.startswith("hybrid") for f in params)


def test_tune_errors_come_before_any_gpu_use(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reached the tables")
    monkeypatch.setattr(C, "_tables_of", boom)
    cases = ((dict(folds=1), "folds >= 2"), (dict(folds=0), "folds >= 2"), (dict(metric="mean_rank"), "ndcg@K, hit_rate@K, mrr"),
             (dict(metric="ndcg@0"), "ndcg@K"), (dict(steps=89), "4095"), (dict(steps=0), ">= 1"))
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            C.evaluate_frame(None, None, 10, [1], 0.5, baseline="hybrid_tuned", hybrid_tune=kw)
    with pytest.raises(ValueError, match="hybrid_tune parameter"):
        C.evaluate_frame(None, None, 10, [1], 0.5, baseline="hybrid_tuned", hybrid_tune={"k": 3})
    with pytest.raises(ValueError, match="hybrid_tune parameter"):     # checked whether or not the system is asked for
        C.evaluate_frame(None, None, 10, [1], 0.5, hybrid_tune={"k": 3})
    with pytest.raises(ValueError, match="for 3 systems"):          # the hybrid's own parameters are the tuned system's
        C.evaluate_frame(None, None, 10, [1], 0.5, baseline="hybrid_tuned", hybrid={"weights": [1, 1]})
    with pytest.raises(ValueError, match="32, 64, 128, 256"):       # and a member's
        C.evaluate_frame(None, None, 10, [1], 0.5, baseline="hybrid_tuned", als={"factors": 100})


# ---- host logic with ops replaced by the restatements ----------------------------------------------------------------
@pytest.fixture
def grid_host_ops(fuse_host_ops, monkeypatch):  # noqa: F811
    """test_fuse_cpu's ``fuse_host_ops`` plus the rank grid and the gain sums as their restatements"""
    def fuse_rank_grid(*a, **kw):
        fuse_host_ops.append("fuse_rank_grid")
        return G.ops_fuse_rank_grid(*a, **kw)
    monkeypatch.setattr(ops, "fuse_rank_grid", fuse_rank_grid)
    monkeypatch.setattr(ops, "rank_gain_rows", BR.ops_rank_gain_rows)
    monkeypatch.setattr(ops, "boot_sums", BR.ops_boot_sums)
    return fuse_host_ops


def test_hybrid_rank_grid_host_logic(grid_host_ops):
    import torch
    rng = np.random.default_rng(3)
    nl, n = 7, 23
    a, b = rng.standard_normal((nl, n)).astype(np.float32), rng.choice(np.float32([0, 1, 2]), (nl, n))
    pop = rng.integers(0, 5, n).astype(np.float32)
    W = rng.random((nl, n)) < 0.3
    W[2] = True                                                  # a list without a target
    wb = CR.pack_bits(W).view(np.int32)
    calls = []

    def src(x):
        def f(l0, l1):
            calls.append((l0, l1))
            return torch.as_tensor(x[l0:l1])
        return f
    sources = [src(a), torch.as_tensor(pop), src(b)]
    grid = recs.hybrid_weight_grid(3, 3)
    tr, ta = np.nonzero(~W)
    pick = rng.permutation(len(tr))[:30]
    for method in ("rrf", "minmax"):
        want, err = G.rank_grid([a, pop, b], grid, R.METHODS[method], 60, tr[pick], ta[pick], n, wb)
        assert err == 0
        for batch in (1, 2, 100):
            calls.clear()
            r = recs.hybrid_rank_grid(sources, wb, tr[pick], ta[pick], grid, method, 60, batch=batch)
            assert r.dtype == torch.int32 and np.array_equal(r.numpy(), want), (method, batch)
            assert batch != 1 or (2, 3) not in calls             # a span that holds no target is not scored
        one = recs.hybrid_rank(sources, wb, tr[pick], ta[pick], grid[5], method, 60)
        assert np.array_equal(one.numpy(), want[5])               # a row of the grid is hybrid_rank with that vector
    assert tuple(recs.hybrid_rank_grid(sources, wb, [], [], grid).shape) == (len(grid), 0)
    st, sa = np.nonzero(W)
    with pytest.raises(ValueError, match="own watched bit"):
        recs.hybrid_rank_grid(sources, wb, [int(st[0])], [int(sa[0])], grid)


def test_evaluate_frame_hybrid_tuned_host_logic(grid_host_ops):
    table = _table()
    U, A, head = _model_of(table.n_users, table.n_anime)
    model = dict(U=U, A=A, head=head, user_ids=table.user_ids, anime_ids=table.anime_ids)
    ks = [1, 5]
    # with the defaults nothing of the feature runs and frame and summary are what they were, key for key
    plain, plain_summary = C.evaluate_frame(model, table, 200, ks, 0.5, baseline="hybrid")
    same, same_summary = C.evaluate_frame(model, table, 200, ks, 0.5, baseline="hybrid",
                                          hybrid_tune={"metric": "mrr", "steps": 3, "folds": 4, "seed": 9})
    assert "fuse_rank_grid" not in grid_host_ops
    assert same.to_csv(index=False) == plain.to_csv(index=False) and same_summary == plain_summary
    assert list(same_summary) == list(plain_summary)
    par = dict(neighbours=4, measure="jaccard", shrink=0.5, min_support=2, min_rating=0.4)
    hyb = dict(systems=("model", "popularity", "itemknn"), method="rrf", rrf_c=10)
    tune = dict(metric="ndcg@5", steps=4, folds=3, seed=7)
    frame, summary = C.evaluate_frame(model, table, 200, ks, 0.5, baseline=("hybrid_tuned", "hybrid"), itemknn=par,
                                      hybrid=hyb, hybrid_tune=tune, ci_replicates=50)
    both = C.evaluate_frame(model, table, 200, ks, 0.5, baseline="hybrid", itemknn=par, hybrid=hyb, ci_replicates=50)
    assert frame[both[0].columns.tolist()].to_csv(index=False) == both[0].to_csv(index=False)
    assert {k: summary[k] for k in both[1]} == both[1]           # the other systems' figures do not move
    assert frame.columns.tolist()[:7] == ["k", "hit_rate", "ndcg", "hit_rate_hybrid", "ndcg_hybrid", "hit_rate_hybrid_tuned",
                                          "ndcg_hybrid_tuned"]
    for col in ("hit_rate_hybrid_tuned_lo", "ndcg_hybrid_tuned_hi", "ndcg_diff_hybrid_tuned", "hit_rate_p_hybrid_tuned"):
        assert col in frame.columns, col
    for key in ("hybrid_tuned_mrr", "hybrid_tuned_mean_rank", "hybrid_tuned_ndcg@5", "hybrid_tuned_mrr_lo",
                "mrr_diff_hybrid_tuned", "mrr_p_hybrid_tuned"):
        assert key in summary, key
    # the same figures from the restatements alone
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
    rows = [grid_of(U, A, users), np.bincount(ta, minlength=table.n_anime).astype(np.float32), knn_rows]
    grid = G.weight_grid(3, 4)
    ranks, err = G.rank_grid(rows, grid, R.RRF, 10, row, anime, table.n_anime, wb)
    assert err == 0 and len(grid) == 16
    want, picks, best_all = G.tuned(ranks, row, len(users), "ndcg@5", table.n_anime, 3, 7)
    b = recs.ranking_metrics(want, ks)
    assert summary["hybrid_tuned_mrr"] == b["mrr"] and summary["hybrid_tuned_mean_rank"] == b["mean_rank"]
    assert frame["hit_rate_hybrid_tuned"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_hybrid_tuned"].tolist() == [b["ndcg"][k] for k in ks]
    assert summary["hybrid_tuned_metric"] == "ndcg@5" and summary["hybrid_tuned_grid"] == 16
    assert summary["hybrid_tuned_fold_weights"] == [grid[i].astype(np.float64).tolist() for i in picks]
    assert summary["hybrid_tuned_weights"] == grid[best_all].astype(np.float64).tolist()
    # row 0 of the grid is the untuned hybrid
    assert recs.ranking_metrics(ranks[0], ks)["mrr"] == summary["hybrid_mrr"]
    # a fold's weights never depend on that fold's own ranks: scramble one fold's targets' ranks and fit again
    fold = G.fold_deal(len(users), 3, 7)
    sums = G.gain_sums(ranks, row, len(users), "ndcg@5", table.n_anime)
    rng = np.random.default_rng(0)
    for f in range(3):
        other = ranks.copy()
        mine = fold[np.asarray(row)] == f
        other[:, mine] = rng.integers(0, table.n_anime, (len(grid), int(mine.sum())))
        assert recs.hybrid_cross_fit(G.gain_sums(other, row, len(users), "ndcg@5", table.n_anime), fold, 3)[f] == picks[f]
    assert recs.hybrid_cross_fit(sums, fold, 3) == picks
