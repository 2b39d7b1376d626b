"""CPU tests of the calibrated-recommendation feature: the restatement of the calibrated re-rank
(tests/calibrate_restatement.py) against the properties its definition promises, the host-side argument checks of
ops.calibrate_rerank / ops.list_calibration / recs.calibrated_topk / anirec_calibrate_rerank / anirec_list_calibration
(none needs a device), the binding, and the calibrated_recs component's flag surface."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import calibrate_restatement as R
from component_cli import load_component
from anime_recommendations_amd import _lib, build, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_list(rng, n, n_cat, density=0.2, levels=8):
    cats = rng.random((n, n_cat)) < density
    score = np.sort(rng.integers(0, levels, n).astype(np.float32) / levels)[::-1].copy()
    profile = rng.integers(0, 50, n_cat)
    return cats, score, profile


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _planted():
    """20 single-category candidates of category 0 (scores 0.9 -> 0.8), 20 of category 1 (0.79 -> 0.7), profile (70, 30)"""
    cats = np.zeros((40, 2), bool)
    cats[:20, 0] = True
    cats[20:, 1] = True
    score = np.concatenate([np.linspace(0.9, 0.8, 20), np.linspace(0.79, 0.7, 20)]).astype(np.float32)
    return cats, score, [70, 30]


def test_c_zero_is_the_stable_descending_order():
    rng = np.random.default_rng(0)
    cats, score, profile = _random_list(rng, 40, 7)
    score = rng.permutation(score)                              # many ties, not sorted
    pos, sc, pen = R.calibrate(cats, score, np.ones(40, bool), profile, 40, 0.0)
    assert pos.tolist() == np.argsort(-score, kind="stable").tolist()
    assert np.array_equal(sc, score[pos])
    # greedy: a shorter k is a prefix
    full = R.calibrate(cats, score, np.ones(40, bool), profile, 40, 0.3)
    part = R.calibrate(cats, score, np.ones(40, bool), profile, 7, 0.3)
    assert all(np.array_equal(f[:7], p, equal_nan=True) for f, p in zip(full, part))


def test_c_one_ignores_scores_except_through_ties():
    rng = np.random.default_rng(1)
    n, n_cat = 30, 6
    cats, score, profile = _random_list(rng, n, n_cat)
    pos, _, pen = R.calibrate(cats, score, np.ones(n, bool), profile, n, 1.0)
    assert sorted(pos.tolist()) == list(range(n))
    q = np.zeros(n_cat, np.int64)
    for s in range(n):
        rest = np.setdiff1d(np.arange(n), pos[:s])
        pens = np.array([R.miscalibration(profile, q + cats[i])[2] for i in rest])
        assert pen[s] == pens.min()                             # every pick takes a least-miscalibrated extension
        assert pos[s] == rest[pens == pens.min()][0]            # and among equals the lowest position
        q += cats[pos[s]]
    # other scores, the same list: val = (0 * score) - pen
    other = R.calibrate(cats, score[::-1].copy() + 3, np.ones(n, bool), profile, n, 1.0)
    assert np.array_equal(other[0], pos) and np.array_equal(_bits(other[2]), _bits(pen))


def test_ties_resolve_by_position():
    n = 6
    cats = np.ones((n, 3), bool)
    pos, _, pen = R.calibrate(cats, np.full(n, 0.5, np.float32), np.ones(n, bool), [1, 2, 3], n, 0.3)
    assert pos.tolist() == list(range(n)) and len(set(pen.tolist())) == 1
    # c = 1: (0 * -1) - pen = -0 - pen and (0 * 1) - pen tie, so position 0 goes first
    pos, _, _ = R.calibrate(cats[:2], np.array([-1, 1], np.float32), np.ones(2, bool), [1, 2, 3], 2, 1.0)
    assert pos.tolist() == [0, 1]
    # a NaN val (0 * inf) sorts after every number, +-inf scores are ordinary numbers
    pos, sc, _ = R.calibrate(cats[:3], np.array([np.inf, 1, -np.inf], np.float32), np.ones(3, bool), [1, 2, 3], 3, 1.0)
    assert pos.tolist() == [1, 0, 2]
    pos, sc, _ = R.calibrate(cats[:3], np.array([-np.inf, 1, np.inf], np.float32), np.ones(3, bool), [1, 2, 3], 3, 0.5)
    assert pos.tolist() == [2, 1, 0]


def test_absent_slots_are_skipped_and_the_row_is_padded():
    cat_bits = np.array([[0b001], [0b010], [0b100], [0b011], [0b111], [0b000], [0b101]], np.uint32)
    idx = np.array([[-1, 2, 4, 3, -1, 6, 5, 5, -1]])
    score = np.array([[9, 1, np.nan, np.nan, 9, np.nan, 2, 2, 9]], np.float32)
    oi, op, os_, open_, err = R.rerank_lists(cat_bits, 3, idx, score, np.array([[1, 1, 1]]), 5, 0.0)
    assert err == 0 and op.tolist() == [[6, 7, 1, -1, -1]] and oi.tolist() == [[5, 5, 2, -1, -1]]   # a repeated index: two
    assert os_[0, :3].tolist() == [2, 2, 1] and np.isnan(os_[0, 3:]).all() and np.isnan(open_[0, 3:]).all()
    assert open_[0, :2].tolist() == [1.0, 1.0]                  # row 5 carries no category: the list says nothing yet
    none = R.calibrate(np.ones((9, 3), bool), score[0], np.zeros(9, bool), [1, 1, 1], 2, 0.3)
    assert none[0].tolist() == [-1, -1] and np.isnan(none[1]).all() and np.isnan(none[2]).all()
    # a bad index or profile entry: the whole list -1 / NaN, the other list untouched
    idx2 = np.array([[0, 1, 2], [0, 7, 2]])
    pr = np.array([[1, 1, 1], [1, 1, 1]])
    oi, op, os_, open_, err = R.rerank_lists(cat_bits, 3, idx2, np.ones((2, 3), np.float32), pr, 2, 0.5)
    assert err == 1 and (oi[1] == -1).all() and np.isnan(open_[1]).all() and (oi[0] >= 0).all()
    for v in (-1, (1 << 24) + 1):
        pr2 = pr.copy()
        pr2[0, 1] = v
        assert R.rerank_lists(cat_bits, 3, idx2[:1], np.ones((1, 3), np.float32), pr2[:1], 2, 0.5)[4] == 1
    pr2[0, 1] = 1 << 24
    assert R.rerank_lists(cat_bits, 3, idx2[:1], np.ones((1, 3), np.float32), pr2[:1], 2, 0.5)[4] == 0


def test_a_zero_profile_gives_pen_zero_and_the_score_order():
    rng = np.random.default_rng(3)
    cats, score, _ = _random_list(rng, 25, 5)
    score = rng.permutation(score)
    for c in (0.3, 0.9):
        pos, _, pen = R.calibrate(cats, score, np.ones(25, bool), [0] * 5, 25, c)
        assert (pen == 0).all() and pos.tolist() == np.argsort(-score, kind="stable").tolist()
    # c = 1: every val is (0 * score) - 0, so the positions decide: the score order of a pool sorted by score
    pos, _, pen = R.calibrate(cats, np.sort(score)[::-1].copy(), np.ones(25, bool), [0] * 5, 25, 1.0)
    assert (pen == 0).all() and pos.tolist() == list(range(25))
    assert R.miscalibration([0, 0], [3, 4]) == (0, 1, np.float32(0))


def test_a_candidate_without_categories_on_an_empty_list_has_pen_one():
    cats = np.array([[False, False], [True, False]])
    pos, _, pen = R.calibrate(cats, np.array([1.0, 0.0], np.float32), np.ones(2, bool), [3, 1], 2, 0.0)
    assert pos.tolist() == [0, 1] and _bits(pen[:1]).tolist() == _bits(np.float32(1.0)).tolist()
    assert pen[1] == np.float32(0.25)                           # (1, 0) tokens against (3/4, 1/4): |3 - 4| + |1 - 0| over 2 * 4
    assert R.miscalibration([3, 1], [0, 0]) == (1, 1, np.float32(1))


@pytest.mark.parametrize("c,first,second,final", [(0.0, 10, 0, np.float32(0.3)), (0.5, 7, 3, np.float32(0.0)),
                                                  (1.0, 7, 3, np.float32(0.0))])
def test_the_planted_two_genre_case(c, first, second, final):
    cats, score, profile = _planted()
    for one in (R.calibrate, R._calibrate_int64):
        pos, _, pen = one(cats, score, np.ones(40, bool), profile, 10, c)
        assert (int((pos < 20).sum()), int((pos >= 20).sum())) == (first, second)
        assert _bits(pen[-1:]).tolist() == _bits(final).tolist()


def test_every_pen_is_the_correctly_rounded_fraction():
    rng = np.random.default_rng(4)
    for n, n_cat, c in ((30, 7, 0.5), (20, 33, 0.1), (12, 1, 1.0)):
        cats, score, profile = _random_list(rng, n, n_cat)
        profile[0] = 1 << 24
        pos, _, pen = R.calibrate(cats, score, np.ones(n, bool), profile, n, c)
        q = np.zeros(n_cat, np.int64)
        P = int(profile.sum())
        for s in range(n):
            q += cats[pos[s]]
            Q = int(q.sum())
            if Q == 0:
                want = np.float32(1.0)
            else:
                tv = sum(abs(Fraction(int(pc), P) - Fraction(int(qc), Q)) for pc, qc in zip(profile, q)) / 2
                want = np.float32(np.float64(tv))               # Fraction -> float64 is correctly rounded
            assert _bits(pen[s:s + 1]).tolist() == _bits(want).tolist(), (n, s)


def test_the_int64_form_is_the_python_int_form():
    """rerank_lists keeps its integers in int64 arrays: the same picks and bits as the Python-int definition"""
    rng = np.random.default_rng(5)
    for n_cat, n, k, c in ((43, 60, 10, 0.5), (5, 20, 20, 1.0), (33, 35, 35, 0.1), (128, 30, 8, 0.3)):
        cw = (n_cat + 31) // 32
        table = np.zeros((90, cw), np.uint32)
        dense = rng.random((90, n_cat)) < min(0.5, 3 / n_cat + 0.02)
        for r, cc in zip(*np.nonzero(dense)):
            table[r, cc >> 5] |= np.uint32(1) << np.uint32(cc & 31)
        idx = rng.integers(-1, 90, (4, n)).astype(np.int32)
        score = np.sort(rng.integers(0, 16, (4, n)).astype(np.float32) / 16, axis=1)[:, ::-1].copy()
        score[1, 3] = np.nan
        profile = rng.integers(0, 50, (4, n_cat))
        profile[2] = 0
        profile[3, 0] = 1 << 24
        a = R.rerank_lists(table, n_cat, idx, score, profile, k, c)
        b = R.rerank_lists(table, n_cat, idx, score, profile, k, c, one=R.calibrate)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(_bits(a[3]), _bits(b[3]))
        # and the list kernel's restatement on every prefix is the re-rank's own pen
        for l in range(4):
            for s in range(k):
                if a[0][l, s] >= 0:
                    got = R.list_calibration(table, n_cat, a[0][l:l + 1, :s + 1], profile[l:l + 1])
                    assert _bits(got[2]).tolist() == _bits(a[3][l, s:s + 1]).tolist()


def test_wrapper_checks_raise_before_any_gpu_use():
    """ValueError (not the no-GPU AnirecError) from shapes and numbers alone: the tensors here live on the host"""
    cat = np.zeros((50, 2), np.uint32)
    ci, cs, pr = torch.zeros(3, 20, dtype=torch.int32), torch.zeros(3, 20), torch.zeros(3, 43, dtype=torch.int32)
    assert _lib.CALIBRATE_MAX_CAND == 1024 and _lib.CALIBRATE_MAX_CAT == 128 and _lib.CALIBRATE_PROFILE_MAX == 1 << 24
    assert ops.check_calibrate(43, 100, 10, 0.5) == (43, 100, 10, 0.5)
    ops.check_calibrate(128, 1024, 1024, 1.0)
    with pytest.raises(ValueError, match="at most 1024"):
        ops.check_calibrate(43, 1025, 10, 0.5)
    with pytest.raises(ValueError, match="at most 1024"):
        ops.calibrate_rerank(cat, 43, torch.zeros(3, 1025, dtype=torch.int32), torch.zeros(3, 1025), pr, 5, 0.5)
    for n_cat in (0, 129, -1):
        with pytest.raises(ValueError, match="1 .. 128"):
            ops.check_calibrate(n_cat, 20, 5, 0.5)
        with pytest.raises(ValueError, match="1 .. 128"):
            ops.list_calibration(cat, n_cat, ci, pr)
    for k in (0, 21):
        with pytest.raises(ValueError, match="1 .. 20"):
            ops.calibrate_rerank(cat, 43, ci, cs, pr, k, 0.5)
    for c in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            ops.calibrate_rerank(cat, 43, ci, cs, pr, 5, c)
    with pytest.raises(ValueError, match="n_lists, n_cand"):
        ops.calibrate_rerank(cat, 43, ci, torch.zeros(3, 19), pr, 5, 0.5)
    with pytest.raises(ValueError, match="cat_bits must be"):
        ops.calibrate_rerank(np.zeros((50, 1), np.uint32), 43, ci, cs, pr, 5, 0.5)
    with pytest.raises(ValueError, match="cat_bits must be"):
        ops.list_calibration(np.zeros((0, 2), np.uint32), 43, ci, pr)
    with pytest.raises(ValueError, match="profile must be"):
        ops.calibrate_rerank(cat, 43, ci, cs, pr[:2], 5, 0.5)
    with pytest.raises(ValueError, match="profile must be"):
        ops.list_calibration(cat, 43, ci, torch.zeros(3, 42, dtype=torch.int32))
    with pytest.raises(ValueError, match="1 .. 1024"):
        ops.list_calibration(cat, 43, torch.zeros(3, 1025, dtype=torch.int32), pr)
    with pytest.raises(ValueError, match="1 .. 1024"):
        ops.list_calibration(cat, 43, torch.zeros(3, 0, dtype=torch.int32), pr)
    U, A, head = torch.zeros(10, 128), torch.zeros(2000, 128), dict(w=1, b=0, gamma=1, beta=0, mov_mean=0, mov_var=1)
    cat_a, pr1 = np.zeros((2000, 2), np.uint32), torch.zeros(1, 43, dtype=torch.int32)
    with pytest.raises(ValueError, match="pool = 5 is smaller than k = 10"):
        recs.calibrated_topk(U, A, head, [0], 10, 5, 0.3, cat_a, 43, pr1)
    with pytest.raises(ValueError, match="pool = 5 is smaller than k = 10"):
        recs.calibrated_topk(U, A, head, [0], 10, 5, 0.0, cat_a, 43, pr1)
    for c in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="calibration"):
            recs.calibrated_topk(U, A, head, [0], 10, 100, c, cat_a, 43, pr1)
    with pytest.raises(ValueError, match="k must be >= 1"):
        recs.calibrated_topk(U, A, head, [0], 0, 100, 0.3, cat_a, 43, pr1)
    with pytest.raises(ValueError, match="at most 1024"):
        recs.calibrated_topk(U, A, head, [0], 10, 1025, 0.3, cat_a, 43, pr1)
    with pytest.raises(ValueError, match="1 .. 128"):
        recs.calibrated_topk(U, A, head, [0], 10, 100, 0.3, cat_a, 129, pr1)
    with pytest.raises(ValueError, match="1 .. 30"):            # the pool is clamped to the 30 anime, k is not
        recs.calibrated_topk(U, A[:30], head, [0], 40, 50, 0.3, cat_a[:30], 43, pr1)


def test_new_symbols_bound_and_entry_point_checks_need_no_gpu():
    assert _lib.PROTOTYPES["anirec_calibrate_max_cand"] == (ctypes.c_size_t, [])
    assert len(_lib.PROTOTYPES["anirec_calibrate_rerank"][1]) == 16
    assert len(_lib.PROTOTYPES["anirec_list_calibration"][1]) == 12
    assert _lib.ABI_VERSION == 5 and "anirec_calibrate.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.anirec_abi_version() == 5 and lib.anirec_calibrate_max_cand() == _lib.CALIBRATE_MAX_CAND == 1024

    def rerank(n_rows=50, n_cat=43, n_lists=0, n_cand=20, k=5, c=0.5, ptr=None):
        return lib.anirec_calibrate_rerank(ptr, n_rows, n_cat, ptr, ptr, ptr, n_lists, n_cand, k, c, ptr, ptr, ptr, ptr,
                                           ptr, None)

    def listcal(n_rows=50, n_cat=43, n_lists=0, k=5, ptr=None):
        return lib.anirec_list_calibration(ptr, n_rows, n_cat, ptr, ptr, n_lists, k, ptr, ptr, ptr, ptr, None)

    fake = 4096         # never followed: every refusal comes before anything is enqueued
    assert rerank() == 0 and rerank(n_cand=1024, k=1024) == 0 and rerank(n_cat=1) == 0 and rerank(n_cat=128) == 0
    assert rerank(c=0.0) == 0 and rerank(c=1.0) == 0            # no lists: nothing to do
    for kw in (dict(n_cat=0), dict(n_cat=129), dict(n_rows=0), dict(n_lists=-1), dict(n_cand=-1), dict(k=0), dict(k=21),
               dict(n_cand=0, k=0), dict(n_cand=1025), dict(c=-0.01), dict(c=1.01), dict(c=float("nan")),
               dict(c=float("inf"))):
        assert rerank(**kw) == -1, kw
        assert rerank(**dict(dict(n_lists=3, ptr=fake), **kw)) == -1, kw
    assert rerank(n_lists=3) == -1                              # NULL buffers with work to do
    assert listcal() == 0 and listcal(k=1024) == 0
    for kw in (dict(n_cat=0), dict(n_cat=129), dict(n_rows=0), dict(n_lists=-1), dict(k=0), dict(k=1025)):
        assert listcal(**kw) == -1, kw
        assert listcal(**dict(dict(n_lists=3, ptr=fake), **kw)) == -1, kw
    assert listcal(n_lists=3) == -1


def test_calibrated_recs_parser_and_mlproject_agree():
    mod, ref = load_component("calibrated_recs"), load_component("model_recs")
    assert mod.STR_FLAGS == ref.STR_FLAGS and mod.BOOL_FLAGS == ref.BOOL_FLAGS       # the model_recs flag set as it is
    defaults = {"calibration": 0.5, "pool": 100, "calibration_column": "Genres", "favorite_percentile": 80}
    assert mod.OPTIONAL_FLAGS == defaults
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert all(getattr(ns, f) == v for f, v in defaults.items()) and ns.model_ID_flow is True
    assert sorted(vars(ns)) == sorted(ref.STR_FLAGS + ref.BOOL_FLAGS + list(defaults))
    ns = parser.parse_args(argv + ["--calibration", "0", "--pool", "40", "--calibration_column", "Source",
                                   "--favorite_percentile", "90"])
    assert (ns.calibration, ns.pool, ns.calibration_column, ns.favorite_percentile) == (0.0, 40, "Source", 90.0)
    for bad in (["--calibration", "1.5"], ["--calibration", "-0.1"], ["--pool", "ten"], ["--calibration_column", "Studios"],
                ["--favorite_percentile", "101"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    with pytest.raises(SystemExit):
        parser.parse_args(argv[2:])
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "calibrated_recs", "MLproject")))
    assert ml["name"] == "calibrated_recs" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    want = list(yaml.safe_load(open(os.path.join(ROOT, "model_recs", "MLproject")))["entry_points"]["main"]["parameters"])
    assert list(params) == want + list(defaults) and sorted(want) == sorted(ref.STR_FLAGS + ref.BOOL_FLAGS)
    assert all(v["description"] for v in params.values()) and all(params[f]["type"] == "str" for f in want)
    assert {k: v["default"] for k, v in params.items() if "default" in v} == defaults
    assert [params[f]["type"] for f in defaults] == ["float", "int", "str", "float"]
    assert main["command"] == "python calibrated_recs.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert os.path.exists(os.path.join(ROOT, "calibrated_recs", "conda.yml"))
