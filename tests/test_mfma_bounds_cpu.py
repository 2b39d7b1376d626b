"""The planted constructions of tests/mfma_restatement.py have teeth (CPU): under the NumPy model of the fp16 MFMA
screening, a window with kEpsMfma keeps every planted neighbour, and at the high score level one with 0.4 kEpsMfma
loses it — so tests/test_mfma_bounds_gpu.py, which runs the same rows through the kernels, fails if the kernels'
window is that much too narrow.  (Random rows cannot show this: their screening errors cancel, and the closest true
neighbour sits nearly 2 eps above the window's lower edge.)"""
import numpy as np
import pytest

import mfma_restatement as mr

f32 = np.float32
KS = (1, 10, 100, 127)


def _table(k, level):
    return mr.planted_table(k, level, 4 if level >= mr.HIGH_LEVEL else 1, 1500, seed=100 + k)


@pytest.mark.parametrize("k", KS)
def test_high_level_plant_binds_the_window_and_a_narrower_one_loses_it(k):
    W, plants = _table(k, mr.HIGH_LEVEL)
    assert not mr.unnorm_flag(W)
    for d in plants:
        r = mr.plant_report(W, d, k)
        # M is the k-th true neighbour, O the (k+1)-th, both at the high level
        assert r["rank_M"] == k - 1 and r["rank_O"] == k
        assert 0.69 <= r["s"][d["M"]] <= 0.95
        assert r["s"][d["M"]] - r["s"][d["O"]] >= 2e-6        # the fp32 chain ranks them like fp64
        # the screening errors of the pair, each at least half the window's eps
        assert r["err_M"] <= -0.5 and r["err_O"] >= 0.5
        # O's overstated score is tau (k_eff-th largest, truncated), and M sits less than 1.2 eps above the edge
        assert r["tau_is_O"]
        assert 3 * mr.ACC / mr.EPS < r["margin_M"] < 1.2 - 3 * mr.ACC / mr.EPS
        assert r["kept"][d["M"]]
        # 0.4 eps: M falls out of the window by more than the hardware's accumulation could move it
        narrow = mr.plant_report(W, d, k, eps=0.4 * mr.EPS)
        assert not narrow["kept"][d["M"]]
        assert narrow["margin_M"] < -3 * mr.ACC / mr.EPS


@pytest.mark.parametrize("level", [0.45, 0.2])
@pytest.mark.parametrize("k", KS)
def test_lower_level_plants_keep_their_neighbour_at_other_tau_exponents(k, level):
    W, (d,) = _table(k, level)
    r = mr.plant_report(W, d, k)
    assert r["rank_M"] == k - 1 and r["rank_O"] == k
    assert abs(r["s"][d["M"]] - level) < 0.01 and r["err_M"] < 0 < r["err_O"]
    assert r["tau_is_O"] and r["kept"][d["M"]] and r["margin_M"] > 3 * mr.ACC / mr.EPS
    # tau is truncated at a lower binade than at the high level
    assert np.floor(np.log2(r["tau"])) < -1


def test_designed_components_keep_their_rounding_through_the_fp32_normalisation():
    rng = np.random.default_rng(3)
    for level in (mr.HIGH_LEVEL, 0.45, 0.2):
        p = mr.plant(10, level, rng)
        for name in ("q", "M", "O"):
            x = p[name]
            dims = np.r_[mr.A_DIMS, mr.B_DIMS, mr.QX] if name == "q" else \
                (mr.A_DIMS if name == "M" else np.r_[mr.B_DIMS, mr.QX])
            assert mr.midpoint_clearance(x[dims]).min() >= mr.MID_MARGIN - 1e-6
            ss = float(np.sum(x.astype(np.float64) ** 2))
            assert abs(ss - 1) < 1e-6
            # k_norm_f16 / k_to_f16 give the same operand; a relative change of 1e-5 (100x what the fp32
            # normalisation of a row this close to unit norm can do) flips no designed rounding
            assert (mr.k_norm_f16(x[None])[0] == mr.k_to_f16(x)).all()
            for rel in (1 - 1e-5, 1 + 1e-5):
                assert (mr.k_to_f16(x[dims] * f32(rel)) == mr.k_to_f16(x[dims])).all()
            # and the sign flip of the negative-slope head is exact
            assert (mr.k_norm_f16(-x[None], -1.0)[0] == mr.k_to_f16(x)).all()


def test_unnorm_edge_rows():
    W, plants = _table(10, mr.HIGH_LEVEL)
    qi, fi = plants[0]["q"], max(d["q"] for d in plants) + 1          # a planted query, a filler row
    for target, flagged in ((1 + 0.9e-3, False), (1 + 1.1e-3, True), (1 - 0.9e-3, False), (1 - 1.1e-3, True)):
        V = W.copy()
        if target > 1:     # the query through its free component (its designed ones stay put)
            V[qi] = mr.with_sumsq(V[qi], target, plants[0]["q_free"])
        else:
            V[fi] = (V[fi] * np.sqrt(target / np.sum(V[fi].astype(np.float64) ** 2))).astype(np.float32)
        r_ = qi if target > 1 else fi
        ss = np.sum(V[r_] * V[r_], dtype=f32)
        assert abs(abs(ss - 1) - abs(target - 1)) < 1e-5   # the fp32 sum lands well clear of the 1e-3 edge
        assert mr.unnorm_flag(V) == flagged
        if not flagged:      # inside the edge: the window still holds for the planted pair
            r = mr.plant_report(V, plants[0], 10)
            assert r["rank_M"] == 9 and r["rank_O"] == 10 and r["tau_is_O"] and r["kept"][plants[0]["M"]]


def test_subnormal_components_stay_inside_eps():
    """Rows with 120 fp16-subnormal components beside 8 dominant ones: the screening error stays within the
    derivation's terms (2^-10 sum |q w| + 2^-25 sum |w|)."""
    rng = np.random.default_rng(5)
    R = np.stack([mr.subnormal_row(rng) for _ in range(64)])
    assert (np.abs(R) < mr.F16_MIN_NORMAL).sum(1).min() >= 120
    err = np.abs(mr.screen(mr.k_to_f16(R), mr.k_to_f16(R)) - mr.exact(R, R))
    absdot = np.abs(R.astype(np.float64)) @ np.abs(R.astype(np.float64)).T
    bound = 2.0 ** -10 * (1 + 2.0 ** -12) * absdot + 2.0 ** -25 * np.abs(R).sum(1)[None, :]
    assert (err <= bound).all() and err.max() < mr.EPS - mr.ACC


def test_p_bound_orders_the_planted_user_complete():
    """model_recs: with O as tau, M's exact rating is above the p_bound of the real window for every activation and
    either slope sign, so a planted user can be proven complete."""
    U, A, plants = mr.predict_split(*_table(10, mr.HIGH_LEVEL))
    d = plants[0]
    r = mr.plant_report(A, d, 10, qvec=U[0])
    assert r["rank_M"] == 9 and r["rank_O"] == 10 and r["tau_is_O"] and r["kept"][d["M"]]
    for act in mr.ACTS:
        for w in (1.7, -1.7):
            hs, hb = mr.head_fold(dict(w=w, b=0.1, gamma=1.0, beta=0.3, mov_mean=0.0, mov_var=1.0))
            sign = -1.0 if hs < 0 else 1.0
            pb = mr.p_bound(r["lo"], mr.EPS, sign, hs, hb, act)
            rating_M = mr.act64(act, sign * r["s"][d["M"]] * hs + hb)
            assert rating_M > pb, (act, w)
