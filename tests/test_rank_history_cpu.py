"""CPU tests of the ranking columns of trainer.fit and of the popularity baseline: the names
schedule.split_rank_metrics takes and refuses, what fit refuses before it touches an engine, recs.popularity_scores
against np.bincount, the new symbol's binding and argument checks, and evaluate_frame's columns and keys without a
baseline."""
import ctypes
import os
import re

import numpy as np
import pytest

from anime_recommendations_amd import _lib, build, components as C, data, recs, schedule, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- names -----------------------------------------------------------------------------------------------------
def test_split_rank_metrics_order_and_case():
    point, specs = schedule.split_rank_metrics(["mse", "Hit_Rate@10", "MAE", "NDCG@5", "mrr", "hit_rate@1", "AUC"])
    assert point == ["mse", "MAE", "AUC"]                                 # as written, in their order
    assert specs == [("hit_rate@10", "hit_rate", 10), ("ndcg@5", "ndcg", 5), ("mrr", "mrr", None),
                     ("hit_rate@1", "hit_rate", 1)]
    assert schedule.split_rank_metrics(("MRR",)) == ([], [("mrr", "mrr", None)])
    assert schedule.split_rank_metrics(["mse"]) == (["mse"], [])
    assert schedule.split_rank_metrics([]) == ([], [])
    assert schedule.split_rank_metrics(["hit_rate@007"])[1] == [("hit_rate@7", "hit_rate", 7)]
    # what resolve_metrics refuses stays its business: a bare string and an unknown name pass through
    assert schedule.split_rank_metrics("mse") == ("mse", [])
    point, specs = schedule.split_rank_metrics(["precision", 3, "ndcg@2"])
    assert point == ["precision", 3] and specs == [("ndcg@2", "ndcg", 2)]
    with pytest.raises(ValueError, match="not supported"):
        schedule.resolve_metrics(point)


@pytest.mark.parametrize("names", [["hit_rate"], ["hit_rate@0"], ["ndcg@x"], ["ndcg"], ["ndcg@"], ["hit_rate@-1"],
                                   ["hit_rate@1.5"], ["mrr@5"], ["hit_rate@5", "HIT_RATE@5"], ["mrr", "MRR"],
                                   ["ndcg@5", "mse", "ndcg@05"], ["hit_rate@ 5"]])
def test_split_rank_metrics_refuses(names):
    with pytest.raises(ValueError, match=r"hit_rate@K and ndcg@K for an integer K >= 1, mrr"):
        schedule.split_rank_metrics(names)


def test_resolve_metrics_still_refuses_the_ranking_names():
    for name in ("hit_rate@5", "ndcg@5", "mrr"):
        with pytest.raises(ValueError, match="not supported"):
            schedule.resolve_metrics([name])


# ---- fit: refused before the engine is touched --------------------------------------------------------------------
class _Untouched:
    """An engine that records every attribute fit reads: fit must refuse before it reads one"""

    def __init__(self, **have):
        object.__setattr__(self, "touched", [])
        object.__setattr__(self, "have", have)

    def __getattr__(self, name):
        if name in self.have:
            return self.have[name]
        if name != "set_epoch_global":                                     # (asking which kind of engine it is)
            self.touched.append(name)
        raise AttributeError(name)


def _table():
    return data.encode_frame(data.synth_user_stats(n_users=40, n_anime=60, n_ratings=1500, seed=3))


def test_fit_columns_follow_the_names():
    """the History keys, as fit lays them out, without running an epoch"""
    table = _table()
    eng = _Untouched()
    cfg = trainer.FitConfig(epochs=0, test_size=200, verbose=0, metrics=("mse", "hit_rate@5", "mae", "NDCG@5", "mrr"),
                            monitor="val_ndcg@5", mode="max")
    # the engine has no metric mask: fit gets past the names, the monitor and the targets and refuses the engine
    with pytest.raises(ValueError, match="the engine accumulates metrics"):
        trainer.fit(table, cfg, engine=eng)


@pytest.mark.parametrize("monitor", ["hit_rate@5", "val_hit_rate@10", "val_ndcg@5", "val_mrr", "mrr", "val_HIT_RATE@5"])
def test_fit_refuses_a_monitor_that_names_no_column(monitor):
    table = _table()
    eng = _Untouched()
    cfg = trainer.FitConfig(epochs=2, test_size=200, verbose=0, metrics=("mse", "HIT_RATE@5"), monitor=monitor,
                            mode="max")
    with pytest.raises(ValueError, match=r"monitor .* names no History column \(loss, mse, val_loss, val_mse, "
                                         r"val_hit_rate@5\)"):
        trainer.fit(table, cfg, engine=eng)
    assert eng.touched == []


def test_fit_refuses_ranking_names_on_a_multi_gpu_engine():
    table = _table()
    eng = _Untouched(set_epoch_global=lambda *a: None)
    cfg = trainer.FitConfig(epochs=2, test_size=200, verbose=0, metrics=("mse", "mrr"), monitor="val_mrr", mode="max")
    with pytest.raises(ValueError, match="multi-GPU"):
        trainer.fit(table, cfg, engine=eng)
    assert eng.touched == []
    # the same engine without a ranking name gets past that check (and is refused for what the stub lacks)
    cfg = trainer.FitConfig(epochs=2, test_size=200, verbose=0, metrics=("mse",))
    with pytest.raises(ValueError, match="optimizer|metrics|engine"):
        trainer.fit(table, cfg, engine=_Untouched(set_epoch_global=lambda *a: None, optimizer="sgd"))


def test_fit_refuses_zero_targets():
    table = _table()
    eng = _Untouched()
    cfg = trainer.FitConfig(epochs=2, test_size=200, verbose=0, metrics=("mse", "ndcg@3"), rank_min_rating=1.5)
    with pytest.raises(ValueError, match="rank_min_rating"):
        trainer.fit(table, cfg, engine=eng)
    assert eng.touched == []
    assert trainer.FitConfig().rank_min_rating == 0.0
    res = trainer.FitResult(history={}, U=None, A=None, head={})
    assert res.rank_seconds == [] and res.rank_baseline == {}


# ---- popularity scores ------------------------------------------------------------------------------------------
def test_popularity_scores_equal_bincount():
    import torch
    rng = np.random.default_rng(8)
    for n_anime, n in ((1, 5), (33, 0), (33, 700), (300, 12_000)):
        a = rng.integers(0, n_anime, n)
        got = recs.popularity_scores(a, n_anime)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (n_anime,)
        np.testing.assert_array_equal(got.numpy(), np.bincount(a, minlength=n_anime).astype(np.float32))
        for cast in (np.int32, np.int64):
            again = recs.popularity_scores(torch.as_tensor(a.astype(cast)), n_anime, n_users=1000)
            assert again.numpy().tobytes() == got.numpy().tobytes()
    with pytest.raises(ValueError, match="out of range"):
        recs.popularity_scores([0, 33], 33)
    with pytest.raises(ValueError, match="out of range"):
        recs.popularity_scores([-1, 3], 33)


def test_popularity_scores_guard_at_two_to_the_24():
    a = np.arange(10)
    assert recs.popularity_scores(a, 10, n_users=(1 << 24) - 1).sum() == 10
    for n_users in (1 << 24, (1 << 24) + 1, 1 << 31):
        with pytest.raises(ValueError, match=r"2\*\*24"):
            recs.popularity_scores(a, 10, n_users=n_users)
    assert float(np.float32((1 << 24) - 1)) == (1 << 24) - 1 and float(np.float32((1 << 24) + 1)) != (1 << 24) + 1


# ---- shared definitions -------------------------------------------------------------------------------------------
def test_held_out_targets_is_one_definition():
    table = _table()
    got = C.held_out_targets(table, 200, 0.6)
    want = recs.held_out_targets(table, 200, 0.6)
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(g, w)
    assert got[3] == want[3]
    users, row, anime, train = want
    _, te = table.split(200)
    take = table.rating[te] >= 0.6
    np.testing.assert_array_equal(users[row], table.user[te][take])
    np.testing.assert_array_equal(anime, table.anime[te][take])
    assert (np.diff(users) > 0).all() and 0 < len(row) < 200
    m = recs.ranking_metrics([0, 3, 9], [1, 5])
    specs = schedule.split_rank_metrics(["mrr", "ndcg@5", "hit_rate@1", "hit_rate@5"])[1]
    assert recs.rank_figures(m, specs) == {"mrr": m["mrr"], "ndcg@5": m["ndcg"][5], "hit_rate@1": m["hit_rate"][1],
                                           "hit_rate@5": m["hit_rate"][5]}
    assert list(recs.rank_figures(m, specs)) == ["mrr", "ndcg@5", "hit_rate@1", "hit_rate@5"]


def test_evaluate_frame_without_a_baseline_is_as_it_was():
    """no held-out row reaches min_rating, so nothing runs on a GPU: the frame's columns and the summary's keys"""
    table = _table()
    head = dict(w=1.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0)
    model = dict(U=np.zeros((table.n_users, 32), np.float32), A=np.zeros((table.n_anime, 32), np.float32), head=head,
                 user_ids=table.user_ids, anime_ids=table.anime_ids)
    keys = ["n", "n_users", "test_size", "min_rating", "mrr", "mean_rank", "median_rank", "hit_rate@1", "ndcg@1",
            "hit_rate@5", "ndcg@5"]
    for kw in ({}, {"baseline": None}):
        frame, summary = C.evaluate_frame(model, table, 200, [5, 1], 1.5, **kw)
        assert frame.columns.tolist() == ["k", "hit_rate", "ndcg"] and frame["k"].tolist() == [1, 5]
        assert list(summary) == keys and summary["n"] == 0
    frame, summary = C.evaluate_frame(model, table, 200, [5, 1], 1.5, baseline="popularity")
    assert frame.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity"]
    assert list(summary) == keys + ["popularity_mrr", "popularity_mean_rank", "popularity_hit_rate@1",
                                    "popularity_ndcg@1", "popularity_hit_rate@5", "popularity_ndcg@5"]
    assert np.isnan(frame["hit_rate_popularity"]).all() and np.isnan(summary["popularity_mrr"])
    for wrong in ("Popularity", "none", "random", ""):
        with pytest.raises(ValueError, match="baseline"):
            C.evaluate_frame(model, table, 200, [1], 1.5, baseline=wrong)


# ---- the entry point ------------------------------------------------------------------------------------------------
def test_score_rank_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert "anirec_score_rank" in set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", src))
    assert len(_lib.PROTOTYPES["anirec_score_rank"][1]) == 10 and _lib.ABI_VERSION == 5
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "anirec_score_rank") and lib.anirec_abi_version() == 5


def test_score_rank_argument_checks_need_no_gpu():
    """the checks made before anything is enqueued, with pointers that are never followed"""
    build.build(verbose=False)
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    call = lambda score=p, n_anime=9, n_users=3, tr=p, ta=p, n_t=4, out=p, err=p: lib.anirec_score_rank(
        score, n_anime, None, n_users, tr, ta, n_t, out, err, None)
    assert call(n_t=0) == 0                                                # nothing to do: OK
    assert call(n_t=0, score=None, tr=None, ta=None, out=None, err=None) == 0
    for kw in (dict(n_anime=0), dict(n_anime=-1), dict(n_users=-1), dict(n_t=-1), dict(score=None), dict(tr=None),
               dict(ta=None), dict(out=None), dict(err=None), dict(n_anime=0, n_t=0), dict(n_users=-1, n_t=0)):
        assert call(**kw) == -1, kw                                        # ANIREC_EINVAL
