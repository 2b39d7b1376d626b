"""CPU tests of the bootstrap: the restatement against the fixtures and the Poisson(1) law it claims,
the coverage of its intervals, the host figures on hand-made sums, the gain tables against ``recs.ranking_metrics``, the
host logic of ``recs.bootstrap_metrics`` / ``components.evaluate_frame`` / ``evaluate_lists_frame`` with ``ops`` replaced by
the restatement, the flag surface and the binding.  The kernels themselves are held to the restatement in
test_boot_gpu.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import boot_restatement as R
from component_cli import load_component
from test_cooc_cpu import _model, _table, host_ops  # noqa: F401  (the other ops as their restatements)

from anime_recommendations_amd import _lib, build, components as C, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P1 = list(recs.POISSON1_THRESHOLDS)
NEW = {"anirec_boot_tile": 0, "anirec_boot_col_tile": 1, "anirec_boot_workspace_bytes": 3, "anirec_rank_gain_rows": 11,
       "anirec_boot_sums": 13, "anirec_boot_weights": 8}
# (seed, b, key) -> r, w: computed apart from this code
FIXTURES = [((0, 1, 0), 0xa53296b4, 1), ((0, 1, 1), 0x7d0ef4c2, 1), ((0, 2, 0), 0xf0858087, 3),
            ((12345, 1000, 349999), 0x34e9f612, 0), ((0xffffffff, 1, 0xffffffff), 0xd768fb30, 2),
            ((7, 65, 64), 0x60bca81d, 1)]


# ---- the draw ------------------------------------------------------------------------------------------------------
def test_the_restatement_gives_the_fixtures_and_the_poisson_thresholds():
    for (seed, b, key), r, w in FIXTURES:
        got = R.draw(seed, b, key)
        assert int(got) == r and int(R.weight(got, P1)) == w, (seed, b, key)
    assert int(R.draw(0xffffffff, 1, -1)) == 0xd768fb30            # the key is the int32 read as uint32
    assert R.poisson1_thresholds() == P1 and len(P1) == 13
    # the same thresholds from the float64 CDF, to the rounding of a double
    cdf = np.cumsum([math.exp(-1.0) / math.factorial(j) for j in range(13)])
    assert np.abs(np.asarray(P1, np.float64) - cdf * 2.0 ** 32).max() < 1.0
    assert R.boot_weights([3, 3, 9], 5, 4, P1)[:, 0].tolist() == R.boot_weights([3, 3, 9], 5, 4, P1)[:, 1].tolist()
    assert R.boot_weights([1, 2, 3], 5, 4, []).sum() == 0
    half = R.boot_weights(np.arange(4000), 5, 4, [0x80000000])
    assert set(np.unique(half)) == {0, 1} and abs(half.mean() - 0.5) < 0.02


def test_the_weights_are_poisson_one_and_uncorrelated():
    n_rep, n_units = 2000, 5000
    W = R.boot_weights(np.arange(n_units), 12345, n_rep, P1).astype(np.float64)
    assert abs(W.mean() - 1.0) < 5e-3 and abs(W.var() - 1.0) < 5e-3
    assert np.abs(W.mean(axis=1) - 1.0).max() < 5.0 / math.sqrt(n_units)
    assert np.abs(W.mean(axis=0) - 1.0).max() < 5.0 / math.sqrt(n_rep)
    hist = np.bincount(W.astype(np.int64).reshape(-1), minlength=14) / W.size
    law = np.asarray([math.exp(-1.0) / math.factorial(j) for j in range(14)])
    assert np.abs(hist - law).max() < 1e-3


def test_the_interval_covers_the_expected_hit_rate():
    """200 trials over one population of 400 units (1-5 targets each, hit probability normal(0.3, 0.15) clipped to
    [0, 1]); a trial draws the hits anew and bootstraps them with seed t.  The units stay, so the interval (which also
    allows for other users) is on the wide side: the share of trials whose 95 % interval holds the expected hit rate
    must lie in [0.90, 1.0]."""
    rng = np.random.default_rng(0)
    n_units, trials, n_rep = 400, 200, 1000
    p = np.clip(rng.normal(0.3, 0.15, n_units), 0.0, 1.0)
    n_t = rng.integers(1, 6, n_units)
    expected = float((p * n_t).sum() / n_t.sum())
    inside = 0
    for t in range(trials):
        values = np.stack([rng.binomial(n_t, p), n_t], axis=1).astype(np.int64)
        sums, err = R.boot_sums(values, np.arange(n_units), t, n_rep, P1)
        f = recs.bootstrap_figures(sums, [1.0], 0.95)
        assert err == 0 and f["n_rep_used"] == n_rep
        inside += f["lo"][0, 0] <= expected <= f["hi"][0, 0]
    print("coverage", inside / trials)
    assert 0.90 <= inside / trials <= 1.0


# ---- the host figures ----------------------------------------------------------------------------------------------
def test_bootstrap_figures_on_hand_made_sums():
    # two systems, one metric at scale 4: figures 0.5 / 0.25 on the sample
    sums = np.asarray([[8, 4, 4], [6, 6, 3], [0, 0, 0], [16, 4, 4], [4, 4, 4], [10, 0, 5]], np.int64)
    f = recs.bootstrap_figures(sums, [4.0], 0.5)
    reps = np.asarray([[0.5, 0.5], [1.0, 0.25], [0.25, 0.25], [0.5, 0.0]])       # the zero-count replicate is dropped
    assert f["n_rep"] == 5 and f["n_rep_used"] == 4
    assert f["value"].tolist() == [[0.5], [0.25]] and f["diff"].tolist() == [[0.25]]
    assert f["se"][:, 0].tolist() == reps.std(axis=0, ddof=1).tolist()
    assert f["lo"][:, 0].tolist() == np.quantile(reps, 0.25, axis=0).tolist()
    assert f["hi"][:, 0].tolist() == np.quantile(reps, 0.75, axis=0).tolist()
    d = reps[:, 0] - reps[:, 1]
    assert f["diff_lo"][0, 0] == np.quantile(d, 0.25) and f["diff_hi"][0, 0] == np.quantile(d, 0.75)
    assert f["p"][0, 0] == min(1.0, 2.0 * (1 + min((d <= 0).sum(), (d >= 0).sum())) / 5.0) == 1.0
    # a first system that always wins: the smallest p the replicates can give
    win = np.asarray([[8, 4, 4]] + [[8 + b, 4, 4] for b in range(99)], np.int64)
    assert recs.bootstrap_figures(win, [4.0])["p"][0, 0] == 2.0 / 100.0
    # a difference that is always 0: p = 1, lo = hi = 0
    same = np.asarray([[8, 8, 4], [6, 6, 3], [2, 2, 4], [9, 9, 5]], np.int64)
    g = recs.bootstrap_figures(same, [4.0])
    assert (g["diff"], g["diff_lo"], g["diff_hi"], g["p"]) == (0.0, 0.0, 0.0, 1.0)
    # fewer than two replicates left: the value stays, the spread is NaN
    few = recs.bootstrap_figures(np.asarray([[8, 4, 4], [6, 6, 3], [0, 0, 0]], np.int64), [4.0])
    assert few["n_rep_used"] == 1 and few["value"].tolist() == [[0.5], [0.25]]
    assert all(np.isnan(few[k]).all() for k in ("se", "lo", "hi", "diff_lo", "diff_hi", "p"))
    none = recs.bootstrap_figures(np.zeros((1, 3), np.int64), [4.0])
    assert none["n_rep"] == 0 and np.isnan(none["value"]).all() and np.isnan(none["diff"]).all()
    one = recs.bootstrap_figures(np.asarray([[8, 4], [6, 3], [2, 4]], np.int64), [4.0])     # one system: no pairs
    assert one["diff"].shape == (0, 1) and one["p"].shape == (0, 1) and one["lo"].shape == (1, 1)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="level"):
            recs.bootstrap_figures(sums, [4.0], bad)
    with pytest.raises(ValueError, match="sums"):
        recs.bootstrap_figures(np.zeros((3, 4), np.int64), [1.0, 1.0])


def test_rank_gain_tables_against_ranking_metrics():
    rng = np.random.default_rng(3)
    ks, n_rows = [10, 1, 50], 700
    tables, names, scales = recs.rank_gain_tables(ks, n_rows)
    assert names == ["hit_rate@1", "hit_rate@10", "hit_rate@50", "ndcg@1", "ndcg@10", "ndcg@50", "mrr", "mean_rank"]
    assert tables.dtype == np.uint32 and tables.shape == (8, n_rows) and scales.tolist() == [2.0 ** 30] * 7 + [1.0]
    assert tables[-1].tolist() == list(range(n_rows)) and tables[0, :2].tolist() == [1 << 30, 0]
    rank = np.concatenate([rng.integers(0, n_rows, 5000), [0, n_rows - 1]])
    want = recs.ranking_metrics(rank, ks)
    got = {n: tables[i][rank].astype(np.int64).sum() / (scales[i] * rank.size) for i, n in enumerate(names)}
    worst = 0.0
    for k in (1, 10, 50):
        worst = max(worst, abs(got["hit_rate@%d" % k] - want["hit_rate"][k]), abs(got["ndcg@%d" % k] - want["ndcg"][k]))
    worst = max(worst, abs(got["mrr"] - want["mrr"]))
    print("largest |delta| of hit rate, ndcg, mrr", worst)
    assert worst <= 2.0 ** -30                                  # each term is off by at most 2**-31
    assert abs(got["mean_rank"] - want["mean_rank"]) <= 1e-9 * want["mean_rank"]
    for bad in ([], [0], [3, -1]):
        with pytest.raises(ValueError, match="k >= 1"):
            recs.rank_gain_tables(bad, 10)
    with pytest.raises(ValueError, match="n_rows"):
        recs.rank_gain_tables([1], 0)


def test_rank_gain_rows_restatement_equals_literal_loops():
    rng = np.random.default_rng(4)
    ranks = rng.integers(-1, 8, (2, 40))
    unit = rng.integers(-1, 6, 40)
    gain = rng.integers(0, 1 << 32, (3, 7), dtype=np.uint64)
    out, err = R.rank_gain_rows(ranks, unit, 5, gain)
    want = np.zeros((5, 7), np.int64)
    for t in range(40):
        if 0 <= unit[t] < 5:
            want[unit[t], -1] += 1
            for s in range(2):
                for m in range(3):
                    if 0 <= ranks[s, t] < 7:
                        want[unit[t], s * 3 + m] += int(gain[m, ranks[s, t]])
    assert err == 1 and (out == want).all()


# ---- host logic with ops replaced by the restatement -----------------------------------------------------------------
@pytest.fixture
def boot_ops(host_ops, monkeypatch):  # noqa: F811
    """``host_ops`` and the three bootstrap wrappers as the restatement; the calls made are logged."""
    def logged(name, fn):
        def call(*a, **kw):
            host_ops.append(name)
            return fn(*a, **kw)
        return call
    for name, fn in dict(rank_gain_rows=R.ops_rank_gain_rows, boot_sums=R.ops_boot_sums,
                         boot_weights=R.ops_boot_weights).items():
        monkeypatch.setattr(ops, name, logged(name, fn))
    return host_ops


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_bootstrap_metrics_host_logic(boot_ops):
    rng = np.random.default_rng(8)
    n_units, n_t, n_rows = 30, 200, 60
    row = rng.integers(0, n_units, n_t)
    a, b = rng.integers(0, n_rows, n_t), rng.integers(0, n_rows, n_t)
    keys = rng.permutation(1000)[:n_units]
    out = recs.bootstrap_metrics({"a": a, "b": b}, row, n_units, [5, 1], n_rep=300, seed=9, level=0.9, unit_key=keys,
                                 n_rows=n_rows, device="cpu")
    assert boot_ops == ["rank_gain_rows", "boot_sums"]
    assert out["metrics"] == ["hit_rate@1", "hit_rate@5", "ndcg@1", "ndcg@5", "mrr", "mean_rank"]
    assert (out["systems"], out["n"], out["n_units"], out["n_rep"], out["n_rep_used"], out["level"], out["seed"]) == \
        (["a", "b"], n_t, n_units, 300, 300, 0.9, 9)
    # from the definition: the weights themselves, the float64 gains, one replicate at a time
    tables, names, scales = recs.rank_gain_tables([1, 5], n_rows)
    W = np.concatenate([np.ones((1, n_units)), R.boot_weights(keys, 9, 300, P1)]).astype(np.int64)
    for sys_name, r in (("a", a), ("b", b)):
        for j, m in enumerate(names):
            fig = [(W[i][row] * tables[j][r].astype(np.int64)).sum() / (scales[j] * W[i][row].sum()) for i in range(301)]
            got = out["figures"][sys_name][m]
            assert got["value"] == fig[0] and math.isclose(got["se"], np.std(fig[1:], ddof=1), rel_tol=1e-12, abs_tol=1e-300)
            assert [got["lo"], got["hi"]] == np.quantile(fig[1:], [(1 - 0.9) / 2, (1 + 0.9) / 2]).tolist()
    want = recs.ranking_metrics(a, [1, 5])
    assert abs(out["figures"]["a"]["mrr"]["value"] - want["mrr"]) <= 2.0 ** -30
    assert abs(out["figures"]["a"]["hit_rate@5"]["value"] - want["hit_rate"][5]) <= 2.0 ** -30
    assert list(out["diffs"]) == ["b"]
    d = out["diffs"]["b"]["mrr"]
    assert d["diff"] == out["figures"]["a"]["mrr"]["value"] - out["figures"]["b"]["mrr"]["value"]
    assert d["lo"] <= d["diff"] <= d["hi"] and 0.0 < d["p"] <= 1.0
    # a subset of the users, under their own keys, re-draws the same weights: the sums of two halves add up
    half = row < 15
    tU = recs.rank_gain_tables([1, 5], n_rows)[0]
    rows = R.rank_gain_rows(np.stack([a, b]), row, n_units, tU)[0]
    whole = R.boot_sums(rows, keys, 9, 50, P1)[0]
    lo = R.boot_sums(R.rank_gain_rows(np.stack([a, b])[:, half], row[half], 15, tU)[0], keys[:15], 9, 50, P1)[0]
    hi = R.boot_sums(R.rank_gain_rows(np.stack([a, b])[:, ~half], row[~half] - 15, 15, tU)[0], keys[15:], 9, 50, P1)[0]
    assert (lo + hi == whole).all()
    # the same system twice: every diff, lo and hi is 0 and every p is 1
    twice = recs.bootstrap_metrics({"a": a, "again": a}, row, n_units, [5], n_rep=50, device="cpu")
    assert all((v["diff"], v["lo"], v["hi"], v["p"]) == (0.0, 0.0, 0.0, 1.0) for v in twice["diffs"]["again"].values())
    # no replicates: the values alone; no targets: NaN and no GPU use
    del boot_ops[:]
    plain = recs.bootstrap_metrics({"a": a}, row, n_units, [5], n_rep=0, device="cpu")
    assert plain["n_rep_used"] == 0 and math.isnan(plain["figures"]["a"]["mrr"]["lo"]) and plain["diffs"] == {}
    assert plain["figures"]["a"]["mean_rank"]["value"] == float(np.mean(a))
    del boot_ops[:]
    empty = recs.bootstrap_metrics({"a": [], "b": []}, [], 0, [5], n_rep=10, n_rows=5, device="cpu")
    assert boot_ops == [] and empty["n"] == 0 and math.isnan(empty["figures"]["a"]["mrr"]["value"])
    # refusals, before any use of ops
    for kw, match in ((dict(n_rep=-1), "n_rep"), (dict(level=0.0), "level"), (dict(level=1.0), "level"),
                      (dict(ks=[0]), "k >= 1"), (dict(ks=[]), "k >= 1")):
        with pytest.raises(ValueError, match=match):
            recs.bootstrap_metrics({"a": a}, row, n_units, **dict(dict(ks=[5], device="cpu"), **kw))
    with pytest.raises(ValueError, match="same"):
        recs.bootstrap_metrics({"a": a, "b": b[:-1]}, row, n_units, [5], device="cpu")
    with pytest.raises(ValueError, match="unit_key"):
        recs.bootstrap_metrics({"a": a}, row, n_units, [5], unit_key=keys[:-1], device="cpu")
    assert boot_ops == []


def test_ops_checks_need_no_device():
    n_rep, table, n_thr = ops.check_boot(7, P1)
    assert (n_rep, n_thr, list(table)) == (7, 13, P1)
    assert ops.check_boot(0, [])[2] == 0 and ops.check_boot(65536, [5, 5])[2] == 2
    for n_rep, thr, match in ((-1, P1, "n_rep"), (65537, P1, "n_rep"), (1, [2, 1], "ascending"), (1, [1 << 32], "ascending"),
                              (1, [-1], "ascending"), (1, list(range(17)), "ascending")):
        with pytest.raises(ValueError, match=match):
            ops.check_boot(n_rep, thr)
    assert ops.boot_limit(100, 13) == R.boot_limit(100, 13) == (1 << 62) // 1300
    assert ops.boot_limit(100, 0) == (1 << 62) // 100 and ops.boot_limit(0, 0) == 1 << 62


def test_evaluate_frame_with_defaults_is_as_it_was_and_gains_the_ci_columns(boot_ops):
    table = _table()
    model = _model(table)
    plain, plain_summary = C.evaluate_frame(model, table, 200, [5, 1], 0.5, baseline="popularity")
    off, off_summary = C.evaluate_frame(model, table, 200, [5, 1], 0.5, baseline="popularity", ci_replicates=0,
                                        ci_level=0.95, ci_seed=0, compare_model=None)
    assert off.to_csv(index=False) == plain.to_csv(index=False) and off_summary == plain_summary
    assert list(off_summary) == list(plain_summary)
    assert plain.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity"]
    assert not {"rank_gain_rows", "boot_sums", "boot_weights"} & set(boot_ops)
    frame, summary = C.evaluate_frame(model, table, 200, [5, 1], 0.5, baseline="popularity", ci_replicates=120,
                                      ci_level=0.9, ci_seed=4)
    assert boot_ops.count("rank_gain_rows") == 1 and boot_ops.count("boot_sums") == 1
    base = plain.columns.tolist()
    assert frame.columns.tolist()[:len(base)] == base
    assert frame[base].to_csv(index=False) == plain.to_csv(index=False)
    new = ["hit_rate_lo", "hit_rate_hi", "hit_rate_diff_popularity", "hit_rate_diff_popularity_lo",
           "hit_rate_diff_popularity_hi", "hit_rate_p_popularity", "ndcg_lo", "ndcg_hi", "ndcg_diff_popularity",
           "ndcg_diff_popularity_lo", "ndcg_diff_popularity_hi", "ndcg_p_popularity", "hit_rate_popularity_lo",
           "hit_rate_popularity_hi", "ndcg_popularity_lo", "ndcg_popularity_hi"]
    assert frame.columns.tolist()[len(base):] == new
    assert list(summary)[:len(plain_summary)] == list(plain_summary)
    assert {k: summary[k] for k in plain_summary} == plain_summary
    assert list(summary)[len(plain_summary):] == [
        "mrr_lo", "mrr_hi", "mrr_diff_popularity", "mrr_diff_popularity_lo", "mrr_diff_popularity_hi", "mrr_p_popularity",
        "mean_rank_lo", "mean_rank_hi", "mean_rank_diff_popularity", "mean_rank_diff_popularity_lo",
        "mean_rank_diff_popularity_hi", "mean_rank_p_popularity", "popularity_mrr_lo", "popularity_mrr_hi",
        "popularity_mean_rank_lo", "popularity_mean_rank_hi", "ci_replicates", "ci_level", "ci_seed", "ci_n_rep_used"]
    assert (summary["ci_replicates"], summary["ci_level"], summary["ci_seed"], summary["ci_n_rep_used"]) == (120, 0.9, 4, 120)
    # the figures are bootstrap_metrics' on the same ranks, the user indices as keys
    users, row, anime, train = recs.held_out_targets(table, 200, 0.5)
    score = recs.popularity_scores(table.anime[train], table.n_anime, table.n_users)
    seen = recs.listed_seen_bits(table.user[train], table.anime[train], users, table.n_users, table.n_anime)
    systems = {"model": (row * 7 + anime * 3) % 11, "popularity": ops.score_rank(score, len(users), row, anime, seen)}
    want = recs.bootstrap_metrics(systems, row, len(users), [1, 5], 120, 4, 0.9, unit_key=users, n_rows=table.n_anime,
                                  device="cpu")
    assert frame["hit_rate_lo"].tolist() == [want["figures"]["model"]["hit_rate@%d" % k]["lo"] for k in (1, 5)]
    assert frame["ndcg_popularity_hi"].tolist() == [want["figures"]["popularity"]["ndcg@%d" % k]["hi"] for k in (1, 5)]
    assert frame["hit_rate_p_popularity"].tolist() == [want["diffs"]["popularity"]["hit_rate@%d" % k]["p"] for k in (1, 5)]
    assert summary["mrr_diff_popularity"] == want["diffs"]["popularity"]["mrr"]["diff"]
    assert summary["popularity_mean_rank_lo"] == want["figures"]["popularity"]["mean_rank"]["lo"]
    assert (frame["hit_rate_lo"] <= frame["hit_rate"] + 2.0 ** -30).all()
    assert (frame["hit_rate"] <= frame["hit_rate_hi"] + 2.0 ** -30).all()
    assert abs(frame["hit_rate_diff_popularity"][0] - (frame["hit_rate"][0] - frame["hit_rate_popularity"][0])) <= 2.0 ** -29


def test_evaluate_frame_compared_with_itself_and_refusals(boot_ops):
    table = _table()
    model = _model(table)
    plain, plain_summary = C.evaluate_frame(model, table, 200, [5, 1], 0.5)
    frame, summary = C.evaluate_frame(model, table, 200, [5, 1], 0.5, compare_model=dict(model))
    assert frame.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_compare", "ndcg_compare"]
    assert frame["hit_rate_compare"].tolist() == plain["hit_rate"].tolist() and summary["compare_mrr"] == plain_summary["mrr"]
    assert boot_ops.count("predict_rank") == 3 and "boot_sums" not in boot_ops
    frame, summary = C.evaluate_frame(model, table, 200, [5, 1], 0.5, compare_model=dict(model), ci_replicates=50)
    for metric in ("hit_rate", "ndcg"):
        for part in ("diff_compare", "diff_compare_lo", "diff_compare_hi"):
            assert frame["%s_%s" % (metric, part)].tolist() == [0.0, 0.0]
        assert frame[metric + "_p_compare"].tolist() == [1.0, 1.0]
        assert frame[metric + "_lo"].tolist() == frame[metric + "_compare_lo"].tolist()
    for metric in ("mrr", "mean_rank"):
        assert [summary["%s_diff_compare%s" % (metric, s)] for s in ("", "_lo", "_hi")] == [0.0, 0.0, 0.0]
        assert summary[metric + "_p_compare"] == 1.0
    del boot_ops[:]
    for kw, match in ((dict(ci_replicates=-1), "n_rep"), (dict(ci_replicates=10, ci_level=1.0), "level"),
                      (dict(ci_replicates=10, ci_level=0.0), "level")):
        with pytest.raises(ValueError, match=match):
            C.evaluate_frame(model, table, 200, [5, 1], 0.5, **kw)
    with pytest.raises(ValueError, match="id tables"):
        C.evaluate_frame(model, table, 200, [5], 0.5, compare_model=dict(model, U=np.zeros((7, 32), np.float32)))
    with pytest.raises(ValueError, match="eval_k"):
        C.evaluate_frame(model, table, 200, [0], 0.5, ci_replicates=10)
    assert boot_ops == []
    # nothing held out: NaN figures, no GPU use
    frame, summary = C.evaluate_frame(model, table, 200, [5], 2.0, ci_replicates=10)
    assert boot_ops == [] and summary["ci_n_rep_used"] == 0 and math.isnan(frame["hit_rate_lo"][0])


def test_evaluate_lists_frame_host_logic(boot_ops, monkeypatch):
    import torch
    table = _table()
    model = _model(table)
    users, row, anime, train = recs.held_out_targets(table, 200, 0.5)
    k = 4

    def diverse_topk(U, A, head, us, k_, pool, d, seen=None):
        boot_ops.append("diverse_topk")
        idx = (np.arange(len(us))[:, None] * 3 + np.arange(k_)[None, :] * (2 + int(d * 10))) % table.n_anime
        return torch.as_tensor(idx.astype(np.int32)), None, None

    def list_quality(Wh, lists, k_=None, target_row=None, target_anime=None, item_count=None, n_raters=None):
        z = torch.zeros(lists.shape, dtype=torch.float32)
        return recs.list_figures(lists, Wh.shape[0], z, z, target_row, target_anime, item_count, n_raters)

    monkeypatch.setattr(recs, "diverse_topk", diverse_topk)
    monkeypatch.setattr(recs, "list_quality", list_quality)
    monkeypatch.setattr(ops, "rownorm", lambda t, device=None: t)
    plain, plain_summary = C.evaluate_lists_frame(model, table, 200, 0.5, [0, 0.3], k=k, pool=10)
    assert plain.columns.tolist() == C.LISTS_COLUMNS and "boot_sums" not in boot_ops
    frame, summary = C.evaluate_lists_frame(model, table, 200, 0.5, [0, 0.3], k=k, pool=10, ci_replicates=80, ci_seed=2)
    extra = [c + s for c in ("hit_rate", "ndcg", "mrr") for s in ("_lo", "_hi", "_diff", "_diff_lo", "_diff_hi", "_p")]
    assert frame.columns.tolist() == C.LISTS_COLUMNS + extra
    assert frame[C.LISTS_COLUMNS].to_csv(index=False) == plain.to_csv(index=False)
    assert {key: summary[key] for key in plain_summary if not _same(summary[key], plain_summary[key])} == {}
    assert summary["lists_ci_n_rep_used"] == 80 and summary["lists_hit_rate_p@0.3"] == frame["hit_rate_p"][1]
    assert [frame[c + s][0] for c in ("hit_rate", "ndcg", "mrr") for s in ("_diff", "_diff_lo", "_diff_hi", "_p")] == \
        [0.0, 0.0, 0.0, 1.0] * 3
    slots = {d: recs.hit_positions(diverse_topk(0, 0, 0, users, k, 10, d)[0], row, anime) for d in (0, 0.3)}
    want = recs.bootstrap_metrics({0: slots[0], 1: slots[0.3]}, row, len(users), [k], 80, 2, unit_key=users, n_rows=k,
                                  device="cpu")
    assert frame["mrr_hi"].tolist() == [want["figures"][i]["mrr"]["hi"] for i in (0, 1)]
    assert frame["hit_rate_diff"][1] == want["diffs"][1]["hit_rate@%d" % k]["diff"]
    assert frame["ndcg_p"][1] == want["diffs"][1]["ndcg@%d" % k]["p"]
    assert abs(want["figures"][1]["hit_rate@%d" % k]["value"] - frame["hit_rate"][1]) <= 2.0 ** -30
    assert abs(want["figures"][1]["mrr"]["value"] - frame["mrr"][1]) <= 2.0 ** -30
    with pytest.raises(ValueError, match="level"):
        C.evaluate_lists_frame(model, table, 200, 0.5, [0], k=k, pool=10, ci_replicates=5, ci_level=2.0)


# ---- the flag surface and the binding ---------------------------------------------------------------------------------
def test_the_ci_flags_are_command_line_only():
    import yaml
    mod = load_component("evaluate")
    assert {f: v[1] for f, v in mod.CI_FLAGS.items()} == {"ci_replicates": 0, "ci_level": 0.95, "ci_seed": 0,
                                                         "compare_model": "none"}
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    ns = mod.make_cli_parser().parse_args(argv)
    assert (ns.ci_replicates, ns.ci_level, ns.ci_seed, ns.compare_model) == (0, 0.95, 0, "none")
    ns = mod.make_cli_parser().parse_args(argv + ["--ci_replicates", "200", "--ci_level", "0.9", "--ci_seed", "7",
                                                   "--compare_model", "other.h5:latest"])
    assert (ns.ci_replicates, ns.ci_level, ns.ci_seed, ns.compare_model) == (200, 0.9, 7, "other.h5:latest")
    plain = mod.make_parser().parse_args(argv)
    assert not any(hasattr(plain, f) for f in mod.CI_FLAGS)
    with pytest.raises(SystemExit):
        mod.make_parser().parse_args(argv + ["--ci_replicates", "200"])
    params = yaml.safe_load(open(os.path.join(ROOT, "evaluate", "MLproject")))["entry_points"]["main"]["parameters"]
    assert not set(mod.CI_FLAGS) & set(params) and not set(mod.CI_FLAGS) & set(mod.OPTIONAL_FLAGS)


def test_new_symbols_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", code))
    for name, arity in NEW.items():
        assert name in declared and len(_lib.PROTOTYPES[name][1]) == arity, name
    assert "#define ANIREC_ABI_VERSION 5" in src and _lib.ABI_VERSION == 5
    assert "anirec_boot.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)


def test_size_queries_and_refusals_need_no_device():
    build.build(verbose=False)
    lib = _lib.load()
    tile = lib.anirec_boot_tile()
    assert tile >= 64 and tile % 64 == 0
    assert lib.anirec_boot_col_tile(0) == 0 and lib.anirec_boot_col_tile(4097) == 0
    assert 1 <= lib.anirec_boot_col_tile(1) <= lib.anirec_boot_col_tile(41) <= 64
    ws = lib.anirec_boot_workspace_bytes
    assert ws(-1, 3, 10) == 0 and ws(5, 0, 10) == 0 and ws(5, 4097, 10) == 0 and ws(5, 3, -1) == 0 and ws(5, 3, 65537) == 0
    assert ws(5, 3, 10) >= 11 * 3 * 8 and ws(0, 3, 10) > 0 and ws(350000, 41, 2000) % (2001 * 41 * 8) == 0
    fake = ctypes.c_void_p(4096)
    good = (ctypes.c_uint32 * 13)(*P1)
    down = (ctypes.c_uint32 * 3)(5, 9, 8)

    def sums(n_units=10, n_col=3, n_rep=5, thr=good, n_thr=13, p=fake, ws_bytes=1 << 30, **null):
        a = dict(values=p, key=p, out=p, err=p, ws=p)
        a.update({k: None for k in null})
        return lib.anirec_boot_sums(a["values"], a["key"], n_units, n_col, 0, n_rep, thr, n_thr, a["out"], a["err"], a["ws"],
                                    ws_bytes, None)
    for kw in (dict(n_units=-1), dict(n_col=0), dict(n_col=4097), dict(n_rep=-1), dict(n_rep=65537), dict(n_thr=17),
               dict(n_thr=-1), dict(thr=down, n_thr=3), dict(thr=None, n_thr=1)):
        assert sums(**kw) == -1, kw
    for name in ("values", "key", "out", "err", "ws"):
        assert sums(**{name: True}) == -1, name
    assert sums(p=ctypes.c_void_p(4100)) == -1                              # int64 buffers are 8-byte aligned
    assert sums(ws_bytes=ws(10, 3, 5) - 1) == -3

    def weights(n_units=10, n_rep=5, thr=good, n_thr=13, p=fake, **null):
        a = dict(key=p, out=p)
        a.update({k: None for k in null})
        return lib.anirec_boot_weights(a["key"], n_units, 0, n_rep, thr, n_thr, a["out"], None)
    for kw in (dict(n_units=-1), dict(n_rep=-1), dict(n_rep=65537), dict(n_thr=17), dict(thr=down, n_thr=3)):
        assert weights(**kw) == -1, kw
    assert weights(n_units=0, p=None) == 0 and weights(n_rep=0, p=None) == 0
    assert weights(key=True) == -1 and weights(out=True) == -1

    def gain(n_sys=2, n_t=10, n_units=4, n_metric=3, n_gain=20, p=fake, **null):
        a = dict(ranks=p, unit=p, gain=p, out=p, err=p)
        a.update({k: None for k in null})
        return lib.anirec_rank_gain_rows(a["ranks"], n_sys, n_t, a["unit"], n_units, a["gain"], n_metric, n_gain, a["out"],
                                         a["err"], None)
    for kw in (dict(n_sys=0), dict(n_metric=0), dict(n_gain=0), dict(n_t=-1), dict(n_units=-1),
               dict(n_sys=64, n_metric=64)):
        assert gain(**kw) == -1, kw
    for name in ("ranks", "unit", "gain", "out", "err"):
        assert gain(**{name: True}) == -1, name
    assert gain(p=ctypes.c_void_p(4100)) == -1
