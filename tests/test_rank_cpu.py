"""CPU tests of the ranking evaluation: recs.ranking_metrics against hand-computed values, the NumPy restatement of
the rank definition (tests/rank_restatement.py) on hand-built ratings, the three new symbols in the header and the
binding, the evaluate component's flag surface and evaluate_frame's id-table check."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import rank_restatement as R
from component_cli import load_component
from anime_recommendations_amd import _lib, build, components as C, data, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("anirec_predict_rank_workspace_bytes", "anirec_predict_rank", "anirec_seen_bits")


def test_ranking_metrics_hand_computed():
    m = recs.ranking_metrics([0, 0, 3, 9, 10, 500], [1, 10, 50])
    assert m["n"] == 6
    assert m["hit_rate"] == {1: 2 / 6, 10: 4 / 6, 50: 5 / 6}
    l2 = math.log2
    want = {1: (1 + 1) / 6, 10: (1 + 1 + 1 / l2(5) + 1 / l2(11)) / 6, 50: (1 + 1 + 1 / l2(5) + 1 / l2(11) + 1 / l2(12)) / 6}
    for k in (1, 10, 50):
        assert abs(m["ndcg"][k] - want[k]) < 1e-15
    assert abs(m["mrr"] - (1 + 1 + 1 / 4 + 1 / 10 + 1 / 11 + 1 / 501) / 6) < 1e-15
    assert m["mean_rank"] == 522 / 6 and m["median_rank"] == 6.0
    # tensors and int32 arrays give the same
    import torch
    assert recs.ranking_metrics(torch.tensor([0, 0, 3, 9, 10, 500], dtype=torch.int32), [1, 10, 50]) == m
    assert recs.ranking_metrics(np.array([0, 0, 3, 9, 10, 500], np.int32), [1, 10, 50]) == m
    r = R.ranking_metrics([0, 0, 3, 9, 10, 500], [1, 10, 50])
    assert r["hit_rate"] == m["hit_rate"] and r["median_rank"] == m["median_rank"]
    assert all(abs(r["ndcg"][k] - m["ndcg"][k]) < 1e-15 for k in (1, 10, 50)) and abs(r["mrr"] - m["mrr"]) < 1e-15


def test_ranking_metrics_empty_and_single():
    m = recs.ranking_metrics([], [1, 5])
    assert m["n"] == 0 and all(math.isnan(m[k]) for k in ("mrr", "mean_rank", "median_rank"))
    assert all(math.isnan(m["hit_rate"][k]) and math.isnan(m["ndcg"][k]) for k in (1, 5))
    m = recs.ranking_metrics(np.zeros(0, np.int32), [3])
    assert m["n"] == 0 and math.isnan(m["hit_rate"][3])
    m = recs.ranking_metrics([2], [1, 3])
    assert m == {"hit_rate": {1: 0.0, 3: 1.0}, "ndcg": {1: 0.0, 3: 0.5}, "mrr": 1 / 3, "mean_rank": 2.0,
                 "median_rank": 2.0, "n": 1}
    with pytest.raises(ValueError):
        recs.ranking_metrics([1, -1], [1])


def test_rank_restatement_on_hand_built_ratings():
    nan = np.float32("nan")
    #                 0    1    2    3     4    5    6    7
    P = np.array([[0.5, 0.9, 0.5, nan, -0.0, 0.0, 0.9, 0.5],
                  [nan, nan, nan, nan, nan, nan, nan, nan]], np.float32)
    key = R.score_key(P[0])
    assert key[3] == 1 and key[5] > key[4] and key[1] == key[6] > key[0] == key[2] == key[7] > key[5]
    # user 0, nothing watched: the order is 1 6 0 2 7 5 4 3 (ties by index, +0 before -0, NaN last)
    order = [1, 6, 0, 2, 7, 5, 4, 3]
    rank, p = R.ranks(P, [0] * 8, list(range(8)))
    assert [int(rank[a]) for a in order] == list(range(8))
    assert np.array_equal(p.view(np.uint32), P[0].view(np.uint32))
    # watched 1 and 2; the target's own flag is ignored: 2 still ranks as if it were unwatched
    w = np.zeros((2, 8), bool)
    w[0, [1, 2]] = True
    rank, _ = R.ranks(P, [0, 0, 0, 0], [6, 2, 7, 3], w)
    assert rank.tolist() == [0, 2, 2, 5]
    # every rating NaN: ranks go by index among the unwatched
    w[1, [0, 4]] = True
    rank, _ = R.ranks(P, [1, 1, 1], [1, 4, 7], w)
    assert rank.tolist() == [0, 3, 5]
    # bits: a packed mask round-trips, bits past n are dropped, seen_bits ors repeats
    assert np.array_equal(R.unpack(R.pack(w), 8), w)
    full = np.full((1, 2), 0xFFFFFFFF, np.uint32)
    assert R.unpack(full, 33).shape == (1, 33)
    b = R.seen_bits([0, 0, 1, 0], [1, 33, 0, 1], 2, 34)
    assert b.tolist() == [[2, 2], [1, 0]]
    assert R.position([4, 2, 7, -1], 7) == 2


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", src))


def test_new_symbols_declared_bound_and_exported():
    names = _declared_functions()
    for n in NEW_SYMBOLS:
        assert n in names, "include/anirec.h does not declare %s" % n
        assert n in _lib.PROTOTYPES, "no ctypes prototype for %s" % n
    assert len(_lib.PROTOTYPES["anirec_predict_rank"][1]) == 18 and len(_lib.PROTOTYPES["anirec_seen_bits"][1]) == 8
    assert _lib.ABI_VERSION == 5
    build.build(verbose=False)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS) and lib.anirec_abi_version() == 5


def test_rank_entry_point_checks_need_no_gpu():
    """the workspace size, the width check and the empty calls return before anything touches a device"""
    build.build(verbose=False)
    lib = _lib.load()
    for dim in _lib.WIDTHS:
        assert lib.anirec_predict_rank_workspace_bytes(300, 7, 65, dim) == (300 + 7) * dim * 4
    assert lib.anirec_predict_rank_workspace_bytes(300, 7, 65, 48) == 0
    assert lib.anirec_predict_rank_workspace_bytes(0, 7, 65, 128) == 0
    h = _lib.Head(1, 0, 1, 0, 0, 1)
    args = lambda dim, n_users, n_t, act=0: (None, None, dim, 300, None, n_users, ctypes.byref(h), act, None, None, None,
                                             n_t, None, None, None, None, 0, None)
    for dim in (0, 16, 48, 100, 512):
        assert lib.anirec_predict_rank(*args(dim, 0, 0)) == -1          # ANIREC_EINVAL, whatever else the call holds
    assert lib.anirec_predict_rank(*args(128, 0, 0, act=9)) == -1
    for dim in _lib.WIDTHS:
        assert lib.anirec_predict_rank(*args(dim, 5, 0)) == 0           # no targets
        assert lib.anirec_predict_rank(*args(dim, 0, 9)) == 0           # no users
    assert lib.anirec_predict_rank(*args(128, 5, 9)) == -1              # NULL tables with work to do


def test_evaluate_parser_and_mlproject_agree():
    mod = load_component("evaluate")
    want = ["input_data", "main_df_type", "model", "model_type", "project_name", "test_size", "eval_k", "min_rating",
            "eval_csv", "eval_type", "ID_emb_name", "anime_emb_name"]
    assert sorted(mod.STR_FLAGS + mod.BOOL_FLAGS) == sorted(want)
    parser = C.make_parser("t", mod.STR_FLAGS, mod.BOOL_FLAGS)
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert all(getattr(ns, f) == "x" for f in mod.STR_FLAGS) and all(getattr(ns, f) is True for f in mod.BOOL_FLAGS)
    with pytest.raises(SystemExit):
        parser.parse_args(argv[2:])
    ml = open(os.path.join(ROOT, "evaluate", "MLproject")).read()
    params = re.findall(r"^      (\w+):\s*$", ml, flags=re.M)
    assert "name: evaluate" in ml and "entry_points:\n  main:" in ml and ml.count("type: str") == len(want)
    assert sorted(params) == sorted(want)
    assert "python evaluate.py" in ml
    for f in want:
        assert "--%s {%s}" % (f, f) in ml
    assert os.path.exists(os.path.join(ROOT, "evaluate", "conda.yml"))
    assert C.literal("[1, 5, 10, 50]") == [1, 5, 10, 50]


def _table(n_users=6, n_anime=9, n=40):
    rng = np.random.default_rng(4)
    return data.RatingTable(rng.integers(0, n_users, n), rng.integers(0, n_anime, n), rng.integers(0, 11, n) / 10.0,
                            np.arange(n_users) + 100, np.arange(n_anime) + 500)


def test_evaluate_frame_refuses_mismatched_id_tables():
    t = _table()
    head = dict(w=1.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0)
    z = lambda r: np.zeros((r, 32), np.float32)
    # another number of users; the message names both shapes
    with pytest.raises(ValueError, match=r"7 users x 9 anime.*6 users x 9 anime"):
        C.evaluate_frame(dict(U=z(7), A=z(9), head=head, user_ids=np.arange(7), anime_ids=t.anime_ids), t, 10, [1], 0.0)
    with pytest.raises(ValueError, match=r"6 users x 8 anime.*6 users x 9 anime"):
        C.evaluate_frame(dict(U=z(6), A=z(8), head=head, user_ids=None, anime_ids=None), t, 10, [1], 0.0)
    # the same shapes, other ids (a model of another data artifact)
    with pytest.raises(ValueError, match="id tables"):
        C.evaluate_frame(dict(U=z(6), A=z(9), head=head, user_ids=t.user_ids[::-1].copy(), anime_ids=t.anime_ids), t, 10,
                         [1], 0.0)
    with pytest.raises(ValueError, match="eval_k"):
        C.evaluate_frame(dict(U=z(6), A=z(9), head=head, user_ids=t.user_ids, anime_ids=t.anime_ids), t, 10, [0, 5], 0.0)


def test_held_out_targets_are_the_validation_rows_at_or_above_min_rating():
    t = _table()
    users, row, anime, train = C.held_out_targets(t, 10, 0.5)
    _, te = t.split(10)
    take = t.rating[te] >= 0.5
    assert train == slice(0, 30) and len(row) == int(take.sum()) == len(anime)
    assert np.array_equal(users[row], t.user[te][take]) and np.array_equal(anime, t.anime[te][take])
    assert np.array_equal(users, np.unique(users))
    users, row, anime, _ = C.held_out_targets(t, 10, 2.0)             # nothing rated that high
    assert len(users) == len(row) == len(anime) == 0
    # no target: NaN metrics and n = 0 without a GPU call
    head = dict(w=1.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0)
    model = dict(U=np.zeros((6, 32), np.float32), A=np.zeros((9, 32), np.float32), head=head, user_ids=t.user_ids,
                 anime_ids=t.anime_ids)
    frame, summary = C.evaluate_frame(model, t, 10, [1, 5], 2.0)
    assert frame["k"].tolist() == [1, 5] and frame.columns.tolist() == ["k", "hit_rate", "ndcg"]
    assert summary["n"] == 0 and frame["hit_rate"].isna().all() and math.isnan(summary["mrr"])
