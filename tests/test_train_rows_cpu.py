"""tests/train_rows.py's row-relative bar bites, shown on the oracles alone (no GPU): the fp32 oracle passes it at the
K the GPU tests use, and a rating dropped from the run of 2 or of 65, a rating of the run of 33 counted twice and two
ratings with their anime index swapped each miss it, with the table and the row named, at widths 32, 64, 128 and 256.
What the table-wide `1e-4 * max|want|` bar of the older tests makes of the same mutated states, kept on record: a
mutation changes the batch statistics, so every touched row moves (by 5e-4 of itself when the batch is one rating
shorter) and misses the row bar, and of those 65 rows per table up to 19 (M) and 31 (V) sit inside the table-wide bar,
being light beside the heaviest row.  In this batch the row a mutation hits directly is never that light: a whole
contribution lost from a touched row is seen by the table-wide bar on M too; what only the row bar sees is a fault that
is small beside its row, and the V of light rows altogether."""
import numpy as np
import pytest

import train_rows as tr

WIDTHS = (32, 64, 128, 256)
TABLE = {"mU": 0, "vU": 0, "mA": 1, "vA": 1}        # moment -> which index array of the batch (ui, ai) addresses it


def test_the_batch_holds_every_run_length_and_leaves_rows_untouched():
    for D in WIDTHS:
        U, A, ui, ai, t = tr.run_length_batch(D, 0)
        assert U.shape == (tr.N_U, D) and A.shape == (tr.N_A, D) and len(ui) == len(ai) == len(t) == tr.N == 2145
        for idx, n_rows in ((ui, tr.N_U), (ai, tr.N_A)):
            runs = tr.run_lengths(idx, n_rows)
            assert sorted(runs[runs > 0].tolist()) == list(range(1, 66)) and (runs[65:] == 0).all()
        assert np.array_equal(tr.run_lengths(ui, tr.N_U)[:65], np.arange(1, 66))
        assert np.abs(U).max() <= 0.05 and np.abs(A).max() <= 0.05 and set(np.unique(t * 10).round().tolist()) <= set(range(11))
        U2, A2, ui2, ai2, t2 = tr.run_length_batch(D, 0)
        assert np.array_equal(ai, ai2) and np.array_equal(U, U2) and np.array_equal(t, t2)      # a pure function
        assert not np.array_equal(ai, tr.run_length_batch(D, 1)[3])


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("optimizer", ["adam", "rmsprop", "adagrad"])
def test_fp32_oracle_passes_the_row_bar(D, optimizer):
    (U, A, ui, ai, t), o32, o64, met, unit = tr.reference(D, optimizer)
    assert sorted(unit) == sorted(tr.MOMENTS if optimizer == "adam" else ("vU", "vA"))
    for k, u in unit.items():
        # the reference alone leaves orders of magnitude below one lost contribution of the longest run
        assert 0 < tr.K * u <= tr.LOST_ONE / 100, (k, u)
        worst = tr.check_rows(o32[k], o64[k], u, tr.K, k, (ui, ai)[TABLE[k]])
        assert worst == pytest.approx(1.0)          # by the unit's definition


@pytest.mark.parametrize("D", WIDTHS)
def test_fp32_oracle_in_another_batch_order_passes_the_row_bar(D):
    """the kernel sums in another order than NumPy (chunks of 32 in sorted order, then the chunks): K must leave room
    for what a change of order alone does to the fp32 oracle.  Five shuffles of the batch; the furthest of 20 was 1.72
    units (train_rows' table)."""
    (U, A, ui, ai, t), o32, o64, met, unit = tr.reference(D)
    rng = np.random.default_rng(D)
    for _ in range(5):
        p = rng.permutation(tr.N)
        st, _ = tr.oracle_step(U, A, ui[p], ai[p], t[p])
        for k in tr.MOMENTS:
            assert tr.check_rows(st[k], o64[k], unit[k], tr.K, k, (ui, ai)[TABLE[k]]) <= tr.K / 2


def test_all_zero_rows_must_be_exactly_zero():
    o64 = np.zeros((3, 8))
    o64[1] = 1.0
    got = o64.astype(np.float32)
    assert tr.check_rows(got, o64, 1e-6, 4.0, "M") == 0.0
    got[2, 5] = 1e-30
    with pytest.raises(tr.RowMiss, match="row 2 is zero") as e:
        tr.check_rows(got, o64, 1e-6, 4.0, "M", idx=np.array([1, 1, 2]))
    assert (e.value.table, e.value.row, e.value.run) == ("M", 2, 1)


# ---- the mutations --------------------------------------------------------------------------------------------
def _drop(run):
    def mutate(ui, ai, t):
        p = int(np.nonzero(ui == run - 1)[0][0])                # the first rating of the run
        keep = np.arange(len(ui)) != p
        return (ui[keep], ai[keep], t[keep]), {0: {run - 1}, 1: {int(ai[p])}}
    return mutate


def _twice(run):
    def mutate(ui, ai, t):
        p = int(np.nonzero(ui == run - 1)[0][0])
        return tuple(np.append(x, x[p]) for x in (ui, ai, t)), {0: {run - 1}, 1: {int(ai[p])}}
    return mutate


def _swap(ui, ai, t):
    p, q = int(np.nonzero(ui == 1)[0][0]), int(np.nonzero(ui == 4)[0][0])    # ratings of the runs of 2 and of 5
    assert ai[p] != ai[q]
    a = ai.copy()
    a[p], a[q] = ai[q], ai[p]
    return (ui, a, t), {0: {1, 4}, 1: {int(ai[p]), int(ai[q])}}


MUTATIONS = {"drop_from_run_of_2": _drop(2), "drop_from_run_of_65": _drop(65), "run_of_33_counts_one_twice": _twice(33),
             "swap_anime_index": _swap}


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("name", list(MUTATIONS))
def test_a_mutated_batch_misses_the_row_bar_where_the_table_wide_bar_passes_light_rows(name, D):
    (U, A, ui, ai, t), o32, o64, met, unit = tr.reference(D)
    (mu, ma, mt), hit = MUTATIONS[name](ui, ai, t)
    bad, _ = tr.oracle_step(U, A, mu, ma, mt)                    # the fp32 step on the mutated batch
    only_new = 0
    for k in tr.MOMENTS:
        idx = (ui, ai)[TABLE[k]]
        with pytest.raises(tr.RowMiss) as e:
            tr.check_rows(bad[k], o64[k], unit[k], tr.K, k, idx)
        # the worst row is a row the mutation touched, named with its table and its run length in the true batch
        assert e.value.table == k and e.value.row in hit[TABLE[k]], (k, e.value.row, hit)
        assert e.value.run == tr.run_lengths(idx, len(o64[k]))[e.value.row] and ("run length %d" % e.value.run) in str(e.value)
        # rows outside the row bar and inside the table-wide one
        ratio, d, m = tr._row_ratio(bad[k], o64[k])
        miss = ratio > tr.K * unit[k]
        old_ok = d <= 1e-4 * m.max()
        assert tr.check_table_wide(bad[k], o64[k], np.nonzero(old_ok)[0])
        only_new += int((miss & old_ok).sum())
        # an untouched row (L2 gradient alone) does not move at all
        assert not miss[65:].any()
    assert only_new > 0, "every row the mutation moved is held by the table-wide bar too"
