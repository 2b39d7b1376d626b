"""CPU tests of the list evaluation: the NumPy restatement of anirec_list_similarity (tests/listeval_restatement.py)
against the properties its definition promises, recs.list_figures (list_quality behind its one kernel call) on hand-made
lists, the host-side argument checks of ops.list_similarity / recs.list_quality / components.evaluate_lists_frame /
anirec_list_similarity (none needs a device), the binding, and the evaluate component's new flags."""
import ctypes
import os

import numpy as np
import pytest
import torch

import listeval_restatement as L
import mmr_restatement as M
from component_cli import load_component
from anime_recommendations_amd import _lib, build, components as C, data, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _sym(rng, n):
    """a symmetric fp32 'similarity' matrix with a unit diagonal"""
    S = np.triu(rng.uniform(-1, 1, (n, n)).astype(np.float32), 1)
    return S + S.T + np.eye(n, dtype=np.float32)


def _literal(S, present):
    """the definition as a plain double loop of float32 scalars: what the restatement's array operations must equal"""
    k = len(present)
    mx, sm = np.full(k, L.NAN32, np.float32), np.full(k, L.NAN32, np.float32)
    with np.errstate(invalid="ignore"):
        for s in range(k):
            if not present[s]:
                continue
            total, largest, first = np.float32(0), np.float32(0), True
            for j in range(s):
                if present[j]:
                    total = np.float32(total + S[s, j])
                    if first or S[s, j] > largest:
                        largest = S[s, j]
                    first = False
            mx[s], sm[s] = largest, total
    return mx, sm


def test_the_restatement_is_the_literal_definition():
    rng = np.random.default_rng(0)
    for k in (1, 2, 7, 40):
        S = _sym(rng, k)
        present = rng.random(k) > 0.2
        if k == 40:                                             # signed zeros and NaNs take the rules' corners
            S[5, :5] = [-0.0, 0.0, -0.0, 0.0, -0.0]
            S[9, 2], S[11, 0], S[12, :12] = np.nan, np.nan, np.nan
            present[[0, 2, 5, 9, 11, 12]] = True
        got, want = L.similarity(S, present), _literal(S, present)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])), k
    assert _bits(got[0])[5] == 0x80000000 and _bits(got[1])[5] == 0        # max keeps the first -0, the sum is 0 + -0 = +0


def test_position_sums_add_up_to_the_triangle():
    """the sum of a list's position sums against the float64 sum of its upper triangle: every position sum is a
    sequential fp32 sum of at most k - 1 terms, so its error is at most (k - 1) * 2**-24 * sum |sim| of ITS terms
    (the standard bound of recursive summation, to first order with the 2**-24 unit roundoff of fp32) — and the errors
    of the positions add"""
    rng = np.random.default_rng(1)
    for k in (2, 10, 65, 300):
        S = _sym(rng, k)
        present = rng.random(k) > 0.1
        mx, sm = L.similarity(S, present)
        pair = present[:, None] & present[None, :] & np.tri(k, k, -1, dtype=bool)
        exact = S.astype(np.float64)[pair].sum()
        bound = (k - 1) * 2.0 ** -24 * np.abs(S.astype(np.float64))[pair].sum()
        got = sm[present].astype(np.float64).sum()
        print("k = %d: |sum - exact| = %.3e, bound %.3e" % (k, abs(got - exact), bound))
        assert abs(got - exact) <= bound
        assert np.isnan(sm[~present]).all() and np.isnan(mx[~present]).all()
        assert np.array_equal(_bits(sm[~present]), np.full((~present).sum(), 0x7FC00000, np.uint32))


def test_sim_max_is_mmr_pen_for_the_same_order():
    """lam = 1 with strictly falling scores picks the present slots in list order: mmr's pen of pick s is sim_max of
    the slot it picked"""
    rng = np.random.default_rng(2)
    for k in (1, 2, 9, 64):
        S = _sym(rng, k)
        present = rng.random(k) > 0.25
        score = np.arange(k, 0, -1).astype(np.float32)
        pos, _, pen = M.mmr(S, score, present, k, 1.0)
        n = int(present.sum())
        assert pos[:n].tolist() == np.flatnonzero(present).tolist() and (pos[n:] == -1).all()
        mx, _ = L.similarity(S, present)
        assert np.array_equal(_bits(mx[pos[:n]]), _bits(pen[:n]))


def test_single_slots_and_empty_lists():
    one = L.similarity(np.ones((1, 1), np.float32), [True])
    assert one[0].tolist() == [0.0] and one[1].tolist() == [0.0]                    # k = 1: nothing before it
    none = L.similarity(np.ones((3, 3), np.float32), [False] * 3)
    assert np.isnan(none[0]).all() and np.isnan(none[1]).all()
    lone = L.similarity(np.ones((3, 3), np.float32), [False, True, False])
    assert lone[0][1] == 0 and lone[1][1] == 0 and np.isnan(lone[0][[0, 2]]).all()
    mx, sm = L.similarity_lists(np.eye(4, dtype=np.float32) * 0.5 + 0.5, np.array([[-1, 2, 2, 3], [1, -1, -1, -1]]))
    assert sm[0, 1:].tolist() == [0.0, 1.0, 1.0] and mx[0, 1:].tolist() == [0.0, 1.0, 0.5]    # a repeated index: two slots
    assert np.isnan(sm[0, 0]) and sm[1, 0] == 0 and np.isnan(sm[1, 1:]).all()


# ---- recs.list_figures: list_quality behind its kernel call, on hand-made lists --------------------------------------
def _figures(idx, n_rows, S=None, **kw):
    """recs.list_figures with the restatement's similarities (``S``: the rows' similarity matrix, 0.5 everywhere by
    default)"""
    idx = np.asarray(idx, np.int32)
    S = np.full((n_rows, n_rows), 0.5, np.float32) if S is None else S
    mx, sm = L.similarity_lists(S, idx)
    return recs.list_figures(torch.from_numpy(idx), n_rows, torch.from_numpy(mx), torch.from_numpy(sm), **kw)


def test_gini_and_coverage():
    n = 6
    equal = _figures([[0, 1, 2], [3, 4, 5], [0, 1, 2], [3, 4, 5]], n)
    assert equal["gini"] == 0.0 and equal["coverage"] == 1.0 and equal["n_lists"] == 4
    hog = _figures([[4], [4], [4]], n)
    assert hog["gini"] == pytest.approx((n - 1) / n, abs=1e-15) and hog["coverage"] == 1 / n
    assert np.isnan(hog["mean_similarity"]) and np.isnan(hog["mean_max_similarity"])      # no list has a pair
    # counts (3, 1, 0, 0, 0, 2) by hand: sorted (0, 0, 0, 1, 2, 3), weights 2 i - 7 = (-5, -3, -1, 1, 3, 5)
    some = _figures([[0, 5, -1], [0, 1, 5], [-1, 0, -1]], n)
    assert some["coverage"] == 3 / n and some["gini"] == pytest.approx((1 * 1 + 3 * 2 + 5 * 3) / (6 * 6), abs=1e-15)
    assert recs.gini([1, 1, 1, 1]) == 0.0 and recs.gini([0, 0, 0, 7]) == pytest.approx(0.75, abs=1e-15)
    assert np.isnan(recs.gini([])) and np.isnan(recs.gini([0, 0]))
    empty = _figures([[-1, -1], [-1, -1]], n)
    assert empty["coverage"] == 0.0 and np.isnan(empty["gini"]) and np.isnan(empty["mean_similarity"])
    nothing = recs.list_figures(torch.zeros(0, 3, dtype=torch.int32), n, None, None, target_row=[], target_anime=[],
                                item_count=np.ones(n), n_raters=4)
    assert nothing["n_lists"] == 0 and nothing["n_targets"] == 0
    assert all(np.isnan(nothing[f]) for f in recs.LIST_FIGURES + recs.HIT_FIGURES)


def test_similarity_figures_from_hand_made_sums():
    S = np.array([[1, .5, .25, 0], [.5, 1, .125, 0], [.25, .125, 1, 0], [0, 0, 0, 1]], np.float32)
    # list 0: rows 0, 1, 2: pairs .5 + .25 + .125 over 3; max per later slot: .5, .25 -> mean .375
    # list 1: rows 2, -1, 0: one pair, .25; list 2: one present slot, not counted
    f = _figures([[0, 1, 2], [2, -1, 0], [-1, 3, -1]], 4, S)
    assert f["mean_similarity"] == ((.5 + .25 + .125) / 3 + .25) / 2
    assert f["mean_max_similarity"] == (.375 + .25) / 2


def test_novelty_from_counts():
    count = np.array([7, 0, 3, 1], np.float32)
    f = _figures([[0, 1, -1], [3, 3, 2]], 4, item_count=count, n_raters=7)
    want = np.mean([-np.log2((c + 1) / 8) for c in (7, 0, 1, 1, 3)])
    assert f["novelty"] == pytest.approx(want, abs=1e-15) and "hit_rate" not in f
    assert "novelty" not in _figures([[0, 1]], 4)
    with pytest.raises(ValueError, match="n_raters"):
        _figures([[0, 1]], 4, item_count=count)
    with pytest.raises(ValueError, match="one count per row"):
        _figures([[0, 1]], 4, item_count=count[:3], n_raters=7)


def test_hit_figures():
    lists = [[5, 3, 9, 3], [1, 2, -1, 4], [7, 7, 7, 7]]
    # every target found: the figures of recs.ranking_metrics on the found positions
    row, anime, pos = [0, 0, 1, 2, 1], [9, 3, 4, 7, 1], [2, 1, 3, 0, 0]       # 3 and 7 are repeated: the lowest slot
    assert recs.hit_positions(torch.tensor(lists), row, anime).tolist() == pos
    f = _figures(lists, 10, target_row=row, target_anime=anime)
    want = recs.ranking_metrics(np.array(pos), [4])
    assert f["hit_rate"] == want["hit_rate"][4] == 1.0 and f["ndcg"] == want["ndcg"][4] and f["mrr"] == want["mrr"]
    assert f["n_targets"] == 5
    # a missing target scores 0 everywhere
    row, anime = [0, 1, 2, 2], [9, 5, 7, 8]
    assert recs.hit_positions(torch.tensor(lists), row, anime).tolist() == [2, -1, 0, -1]
    f = _figures(lists, 10, target_row=row, target_anime=anime)
    assert f["hit_rate"] == 0.5 and f["ndcg"] == (1 / np.log2(4) + 1) / 4 and f["mrr"] == (1 / 3 + 1) / 4
    for bad_row, bad_anime in (([3], [1]), ([-1], [1]), ([0], [-1]), ([0, 1], [1])):
        with pytest.raises(ValueError, match="target"):
            _figures(lists, 10, target_row=bad_row, target_anime=bad_anime)
    with pytest.raises(ValueError, match="come together"):
        _figures(lists, 10, target_row=[0])


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_wrapper_checks_raise_before_any_gpu_use():
    """ValueError (not the no-GPU AnirecError) from shapes and numbers alone: the tensors here live on the host"""
    What = torch.zeros(50, 128)
    with pytest.raises(ValueError, match="257 slots per list, 1 .. 256 at width 128"):
        ops.list_similarity(What, torch.zeros(3, 257, dtype=torch.int32))
    for dim, cap in ((32, 1024), (64, 512), (128, 256), (256, 128)):
        assert ops.check_list_similarity(dim, cap) == (dim, cap) and ops.check_list_similarity(dim, 1) == (dim, 1)
        with pytest.raises(ValueError, match="1 .. %d at width %d" % (cap, dim)):
            ops.check_list_similarity(dim, cap + 1)
        with pytest.raises(ValueError, match="1 .. %d" % cap):
            ops.check_list_similarity(dim, 0)
    with pytest.raises(ValueError, match="embedding_size"):
        ops.list_similarity(torch.zeros(50, 48), torch.zeros(3, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[n_lists, k\]"):
        ops.list_similarity(What, torch.zeros(15, dtype=torch.int32))
    with pytest.raises(ValueError, match="no rows"):
        ops.list_similarity(torch.zeros(0, 128), torch.zeros(3, 5, dtype=torch.int32))
    lists = torch.zeros(3, 300, dtype=torch.int32)
    with pytest.raises(ValueError, match="1 .. 256 at width 128"):
        recs.list_quality(What, lists)
    for k in (0, 301):
        with pytest.raises(ValueError, match="1 .. 300"):
            recs.list_quality(What, lists, k)
    with pytest.raises(ValueError, match=r"\[n_lists, k\]"):
        recs.list_quality(What, lists[0])
    empty = recs.list_quality(What, lists[:0], 10, target_row=[], target_anime=[])           # no lists: no device either
    assert empty["n_lists"] == 0 and np.isnan(empty["coverage"]) and np.isnan(empty["hit_rate"])


def _table(n_users=6, n_anime=9, n=40):
    rng = np.random.default_rng(4)
    return data.RatingTable(rng.integers(0, n_users, n), rng.integers(0, n_anime, n), rng.integers(0, 11, n) / 10.0,
                            np.arange(n_users) + 100, np.arange(n_anime) + 500)


def test_evaluate_lists_frame_checks_raise_before_any_gpu_use():
    t = _table()
    head = dict(w=1.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0)
    z = lambda r: np.zeros((r, 32), np.float32)
    good = dict(U=z(6), A=z(9), head=head, user_ids=t.user_ids, anime_ids=t.anime_ids)
    with pytest.raises(ValueError, match=r"7 users x 9 anime.*6 users x 9 anime"):
        C.evaluate_lists_frame(dict(good, U=z(7), user_ids=np.arange(7)), t, 10, 0.0, [0.3])
    with pytest.raises(ValueError, match="id tables"):
        C.evaluate_lists_frame(dict(good, user_ids=t.user_ids[::-1].copy()), t, 10, 0.0, [0.3])
    for ds in ([-0.1], [0, 1.5], [float("nan")], []):
        with pytest.raises(ValueError, match="lists_diversity"):
            C.evaluate_lists_frame(good, t, 10, 0.0, ds)
    with pytest.raises(ValueError, match="lists_k must be >= 1"):
        C.evaluate_lists_frame(good, t, 10, 0.0, [0.3], k=0)
    with pytest.raises(ValueError, match="lists_pool = 5 is smaller than lists_k = 6"):
        C.evaluate_lists_frame(good, t, 10, 0.0, [0.3], k=6, pool=5)
    # nothing held out at or above min_rating: NaN rows, no device
    frame, summary = C.evaluate_lists_frame(good, t, 10, 2.0, [0, 0.25], k=3, pool=5)
    assert frame.columns.tolist() == C.LISTS_COLUMNS and frame["diversity"].tolist() == [0.0, 0.25]
    assert frame["k"].tolist() == [3, 3] and frame["pool"].tolist() == [5, 5] and frame.iloc[:, 3:].isna().all().all()
    assert sorted(summary) == sorted("lists_%s@%s" % (c, d) for c in C.LISTS_COLUMNS[3:] for d in ("0", "0.25"))


def test_new_symbol_bound_and_entry_point_checks_need_no_gpu():
    assert len(_lib.PROTOTYPES["anirec_list_similarity"][1]) == 10
    assert _lib.ABI_VERSION == 5 and "anirec_listeval.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.anirec_abi_version() == 5

    def call(dim=128, n_rows=50, n_lists=0, k=5, ptr=None):
        return lib.anirec_list_similarity(ptr, dim, n_rows, ptr, n_lists, k, ptr, ptr, ptr, None)

    for dim in _lib.WIDTHS:
        assert call(dim=dim) == 0 and call(dim=dim, k=32768 // dim) == 0       # no lists: nothing to do
        assert call(dim=dim, k=32768 // dim + 1) == -1
    fake = 4096         # never followed: every refusal comes before anything is enqueued
    for kw in (dict(dim=48), dict(dim=0), dict(dim=-32), dict(n_rows=0), dict(n_rows=-1), dict(n_lists=-1), dict(k=0),
               dict(k=-1), dict(k=257)):
        assert call(**kw) == -1, kw
        assert call(**dict(dict(n_lists=3, ptr=fake), **kw)) == -1, kw
    assert call(n_lists=3) == -1                                # NULL buffers with work to do


def test_evaluate_parser_and_mlproject_agree_on_the_lists_flags():
    mod = load_component("evaluate")
    want = {"lists_diversity": "none", "lists_k": 10, "lists_pool": 100, "lists_csv": "eval_lists.csv"}
    assert {f: v[1] for f, v in mod.OPTIONAL_FLAGS.items()} == want and len(mod.STR_FLAGS) == 12
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    ns = parser.parse_args(argv)
    assert {f: getattr(ns, f) for f in want} == want and ns.baseline == "none"
    assert sorted(vars(ns)) == sorted(mod.STR_FLAGS + ["baseline"] + list(want))
    ns = parser.parse_args(argv + ["--lists_diversity", "[0, 0.1, 0.3]", "--lists_k", "5", "--lists_pool", "40",
                                   "--lists_csv", "l.csv"])
    assert C.literal(ns.lists_diversity) == [0, 0.1, 0.3] and (ns.lists_k, ns.lists_pool, ns.lists_csv) == (5, 40, "l.csv")
    with pytest.raises(SystemExit):
        parser.parse_args(argv + ["--lists_k", "ten"])
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "evaluate", "MLproject")))
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + ["baseline"] + list(want)
    assert {f: params[f]["default"] for f in want} == want and all(params[f]["description"] for f in want)
    assert all("type" not in params[f] for f in want)
    assert main["command"] == "python evaluate.py " + " ".join("--%s {%s}" % (f, f) for f in params)
