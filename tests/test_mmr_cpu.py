"""CPU tests of the diversified-recommendation feature: the NumPy restatement of the MMR re-rank (tests/mmr_restatement.py)
against the properties its definition promises, the host-side argument checks of ops.mmr_rerank / recs.diverse_topk /
anirec_mmr_rerank (none needs a device), the binding, and the diverse_recs component's flag surface."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mmr_restatement as M
from component_cli import load_component
from anime_recommendations_amd import _lib, build, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sym(rng, n):
    """a symmetric fp32 'similarity' matrix with a unit diagonal"""
    S = rng.uniform(-1, 1, (n, n)).astype(np.float32)
    S = np.triu(S, 1)
    return S + S.T + np.eye(n, dtype=np.float32)


def test_lam_one_is_the_stable_descending_order():
    rng = np.random.default_rng(0)
    n = 40
    score = rng.integers(0, 8, n).astype(np.float32) / 4 - 1          # many ties, both signs, -0 is not among them
    pos, sc, pen = M.mmr(_sym(rng, n), score, np.ones(n, bool), n, 1.0)
    assert pos.tolist() == np.argsort(-score, kind="stable").tolist()
    assert np.array_equal(sc, score[pos]) and pen[0] == 0
    # greedy: a shorter k is a prefix
    S = _sym(rng, n)
    full = M.mmr(S, score, np.ones(n, bool), n, 0.3)
    part = M.mmr(S, score, np.ones(n, bool), 7, 0.3)
    assert all(np.array_equal(f[:7], p, equal_nan=True) for f, p in zip(full, part))


def test_lam_zero_always_takes_a_least_similar_candidate():
    rng = np.random.default_rng(1)
    n = 30
    S = _sym(rng, n)
    score = rng.uniform(0.1, 1, n).astype(np.float32)
    pos, _, pen = M.mmr(S, score, np.ones(n, bool), n, 0.0)
    assert pos[0] == 0 and pen[0] == 0                          # every val is 0 before the first pick: position decides
    assert sorted(pos.tolist()) == list(range(n))
    for s in range(1, n):
        rest = np.setdiff1d(np.arange(n), pos[:s])
        pens = S[np.ix_(rest, pos[:s])].max(axis=1)             # each unpicked candidate's largest S to a picked one
        assert pen[s] == pens.min() == S[pos[s], pos[:s]].max()
        assert pos[s] == rest[pens == pens.min()][0]            # and among equals the lowest position


def test_ties_resolve_by_position():
    n = 6
    S = np.full((n, n), 0.25, np.float32)
    pos, _, pen = M.mmr(S, np.full(n, 0.5, np.float32), np.ones(n, bool), n, 0.3)
    assert pos.tolist() == list(range(n)) and pen.tolist() == [0.0] + [0.25] * (n - 1)
    # lam = 0: (0 * -1) - (1 * 0) = -0 and (0 * 1) - 0 = +0 tie, so position 0 goes first
    pos, _, _ = M.mmr(np.eye(2, dtype=np.float32), np.array([-1, 1], np.float32), np.ones(2, bool), 2, 0.0)
    assert pos.tolist() == [0, 1]
    # a NaN val (inf - inf) sorts after every number, +-inf scores are ordinary numbers
    S = np.array([[1, np.inf, 0], [np.inf, 1, 0], [0, 0, 1]], np.float32)
    pos, sc, _ = M.mmr(S, np.array([np.inf, np.inf, -np.inf], np.float32), np.ones(3, bool), 3, 0.5)
    assert pos.tolist() == [0, 2, 1] and sc.tolist() == [np.inf, -np.inf, np.inf]


def test_absent_slots_are_skipped_and_the_row_is_padded():
    rng = np.random.default_rng(2)
    What = rng.normal(size=(9, 8)).astype(np.float32)
    What[4] = np.nan                                            # a zero row, normalised
    What[6, 3] = np.inf
    idx = np.array([[-1, 2, 4, 3, -1, 6, 5, 5, -1]])
    score = np.array([[9, 1, 9, np.nan, 9, 9, 2, 2, 9]], np.float32)
    pres = M.present_mask(What, idx, score)
    assert pres.tolist() == [[False, True, False, False, False, False, True, True, False]]
    S = np.eye(9, dtype=np.float32)
    oi, op, os_, open_ = M.rerank_lists(S, What, idx, score, 5, 1.0)
    assert op.tolist() == [[6, 7, 1, -1, -1]] and oi.tolist() == [[5, 5, 2, -1, -1]]       # a repeated index: two candidates
    assert os_[0, :3].tolist() == [2, 2, 1] and np.isnan(os_[0, 3:]).all() and np.isnan(open_[0, 3:]).all()
    assert open_[0, :3].tolist() == [0, 1, 0]                   # the twin's similarity to its first copy is S[5, 5]
    none = M.mmr(S, score[0], np.zeros(9, bool), 2, 0.3)
    assert none[0].tolist() == [-1, -1] and np.isnan(none[1]).all() and np.isnan(none[2]).all()


def test_wrapper_checks_raise_before_any_gpu_use():
    """ValueError (not the no-GPU AnirecError) from shapes and numbers alone: the tensors here live on the host"""
    What = torch.zeros(50, 128)
    ci, cs = torch.zeros(3, 20, dtype=torch.int32), torch.zeros(3, 20)
    with pytest.raises(ValueError, match="at most 256 at width 128"):
        ops.mmr_rerank(What, torch.zeros(3, 257, dtype=torch.int32), torch.zeros(3, 257), 5, 0.5)
    for dim, cap in ((32, 1024), (64, 512), (128, 256), (256, 128)):
        assert _lib.mmr_max_cand(dim) == cap
        ops.check_mmr(dim, cap, cap, 1.0)
        with pytest.raises(ValueError, match="at most %d" % cap):
            ops.check_mmr(dim, cap + 1, 1, 1.0)
    with pytest.raises(ValueError, match="1 .. 20"):
        ops.mmr_rerank(What, ci, cs, 21, 0.5)
    with pytest.raises(ValueError, match="1 .. 20"):
        ops.mmr_rerank(What, ci, cs, 0, 0.5)
    for lam in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            ops.mmr_rerank(What, ci, cs, 5, lam)
    with pytest.raises(ValueError, match="embedding_size"):
        ops.mmr_rerank(torch.zeros(50, 48), ci, cs, 5, 0.5)
    with pytest.raises(ValueError, match="n_lists, n_cand"):
        ops.mmr_rerank(What, ci, torch.zeros(3, 19), 5, 0.5)
    U, A, head = torch.zeros(10, 128), torch.zeros(2000, 128), dict(w=1, b=0, gamma=1, beta=0, mov_mean=0, mov_var=1)
    with pytest.raises(ValueError, match="pool = 5 is smaller than k = 10"):
        recs.diverse_topk(U, A, head, [0], 10, 5, 0.3)
    with pytest.raises(ValueError, match="pool = 5 is smaller than k = 10"):
        recs.diverse_topk(U, A, head, [0], 10, 5, 0.0)
    for d in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="diversity"):
            recs.diverse_topk(U, A, head, [0], 10, 100, d)
    with pytest.raises(ValueError, match="k must be >= 1"):
        recs.diverse_topk(U, A, head, [0], 0, 100, 0.3)
    with pytest.raises(ValueError, match="at most 256 at width 128"):
        recs.diverse_topk(U, A, head, [0], 10, 300, 0.3)
    with pytest.raises(ValueError, match="1 .. 30"):            # the pool is clamped to the 30 anime, k is not
        recs.diverse_topk(U, A[:30], head, [0], 40, 50, 0.3)


def test_new_symbols_bound_and_entry_point_checks_need_no_gpu():
    assert len(_lib.PROTOTYPES["anirec_mmr_max_cand"][1]) == 1 and len(_lib.PROTOTYPES["anirec_mmr_rerank"][1]) == 15
    assert _lib.PROTOTYPES["anirec_mmr_max_cand"][0] is ctypes.c_size_t
    assert _lib.ABI_VERSION == 5 and "anirec_mmr.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.anirec_abi_version() == 5
    for dim in _lib.WIDTHS:
        assert lib.anirec_mmr_max_cand(dim) == _lib.mmr_max_cand(dim) == 32768 // dim
    for dim in (0, 16, 48, 100, 512, -32):
        assert lib.anirec_mmr_max_cand(dim) == 0

    def call(dim=128, n_rows=50, n_lists=0, n_cand=20, k=5, lam=0.5, ptr=None):
        return lib.anirec_mmr_rerank(ptr, dim, n_rows, ptr, ptr, n_lists, n_cand, k, lam, ptr, ptr, ptr, ptr, ptr, None)

    for dim in _lib.WIDTHS:
        assert call(dim=dim) == 0 and call(dim=dim, n_cand=32768 // dim, k=32768 // dim) == 0      # no lists: nothing to do
        assert call(dim=dim, n_cand=32768 // dim + 1) == -1
    fake = 4096         # never followed: every refusal comes before anything is enqueued
    for kw in (dict(dim=48), dict(dim=0), dict(n_rows=0), dict(n_lists=-1), dict(n_cand=-1), dict(k=0), dict(k=21),
               dict(n_cand=0, k=0), dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan")), dict(lam=float("inf"))):
        assert call(**kw) == -1, kw
        assert call(**dict(dict(n_lists=3, ptr=fake), **kw)) == -1, kw
    assert call(n_lists=3) == -1                                # NULL buffers with work to do
    assert call(lam=0.0) == 0 and call(lam=1.0) == 0


def test_diverse_recs_parser_and_mlproject_agree():
    mod, ref = load_component("diverse_recs"), load_component("model_recs")
    assert mod.STR_FLAGS == ref.STR_FLAGS and mod.BOOL_FLAGS == ref.BOOL_FLAGS       # the model_recs flag set as it is
    assert mod.OPTIONAL_FLAGS == {"diversity": 0.3, "pool": 100}
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert ns.diversity == 0.3 and ns.pool == 100 and ns.model_ID_flow is True
    assert sorted(vars(ns)) == sorted(ref.STR_FLAGS + ref.BOOL_FLAGS + ["diversity", "pool"])
    ns = parser.parse_args(argv + ["--diversity", "0", "--pool", "40"])
    assert ns.diversity == 0.0 and ns.pool == 40
    for bad in (["--diversity", "1.5"], ["--diversity", "-0.1"], ["--pool", "ten"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    with pytest.raises(SystemExit):
        parser.parse_args(argv[2:])
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "diverse_recs", "MLproject")))
    assert ml["name"] == "diverse_recs" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    want = list(yaml.safe_load(open(os.path.join(ROOT, "model_recs", "MLproject")))["entry_points"]["main"]["parameters"])
    assert list(params) == want + ["diversity", "pool"] and sorted(want) == sorted(ref.STR_FLAGS + ref.BOOL_FLAGS)
    assert all(v["description"] for v in params.values()) and all(params[f]["type"] == "str" for f in want)
    assert {k: v["default"] for k, v in params.items() if "default" in v} == {"diversity": 0.3, "pool": 100}
    assert (params["diversity"]["type"], params["pool"]["type"]) == ("float", "int")
    assert main["command"] == "python diverse_recs.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert os.path.exists(os.path.join(ROOT, "diverse_recs", "conda.yml"))
