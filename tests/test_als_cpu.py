"""CPU tests of implicit-feedback ALS: the restatement against linear algebra, the recorded fp32
distances the GPU tests take their tolerances from, the argument rules and size queries of the C entry points, and the
flag surface of ``--baseline als``."""
import ctypes

import numpy as np
import pytest

import als_cases as K
import als_restatement as R
from anime_recommendations_amd import _lib, build, components as C, ops, recs
from component_cli import load_component


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


# ---- the definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", K.WIDTHS)
@pytest.mark.parametrize("pair", (0, 1))
def test_fp64_iteration_run_to_convergence_solves_the_normal_equations(dim, pair):
    alpha, lam = K.PAIRS[pair]
    Y = K.table(dim)
    off, idx, w, start = K.rows(dim)
    G = R.gram64(Y)
    for per in (False, True):
        ex = None if not per else alpha * w.astype(np.float64)
        for u, (i, e) in enumerate(R.row_lists(off, idx, ex, alpha, np.float64)):
            if len(i) == 0:
                continue
            A, b = R.normal_equations(Y, i, e, lam)
            want = np.linalg.solve(A, b)
            # run past the definition's exit (to r . r <= 1e-30 of its first value) to convergence: in floating point
            # CG needs more than dim steps
            # (the 16-entry row at width 64 and (40, 0.1) is 2e-8 away after dim + 20 steps, 2e-14 after 120)
            x, _ = R.row64(Y, G, i, e, lam, start[u], 2 * dim + 40, rtol2=1e-30)
            assert np.abs(x - want).max() <= 1e-8, (u, len(i), np.abs(x - want).max())


def test_row_loss_equals_the_sum_over_all_items():
    for dim in (32, 128):
        Y = K.table(dim)
        off, idx, w, start = K.rows(dim)
        G = R.gram64(Y)
        for alpha, lam in K.PAIRS:
            for u, (i, e) in enumerate(R.row_lists(off, idx, alpha * w.astype(np.float64), alpha, np.float64)):
                if u == K.LONG_ROW:
                    continue                                     # repeats: the list is no set of items
                x, loss = R.row64(Y, G, i, e, lam, start[u], 2)
                if len(i) == 0:
                    assert loss == 0.0 and not x.any()
                    continue
                want = R.objective_brute(Y, i, e, lam, x)
                assert abs(loss - want) <= 1e-12 * max(1.0, abs(want)), (dim, u)


def test_total_loss_of_an_fp64_fit_never_rises():
    u, i = K.fit_pairs()
    par = dict(K.FIT, sweeps=6)
    X, Y, losses = R.fit(u, i, dtype=np.float64, **par)
    assert len(losses) == 12 and all(b <= a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < 0.2 * losses[0]
    # the reported loss is the objective itself, summed over all pairs
    like = np.zeros((K.FIT["n_users"], K.FIT["n_items"]))
    like[u, i] = 1.0
    c = 1.0 + K.FIT["alpha"] * like
    want = (c * (like - X @ Y.T) ** 2).sum() + K.FIT["reg"] * ((X ** 2).sum() + (Y ** 2).sum())
    assert abs(losses[-1] - want) <= 1e-10 * want


def test_planted_blocks_fp64_als_beats_popularity_by_a_wide_gap():
    tu, ti, hu, hi = K.block_pairs()
    X, Y, _ = R.fit(tu, ti, dtype=np.float64, **K.BLOCK)
    pop = np.tile(np.bincount(ti, minlength=K.BLOCK["n_items"]).astype(np.float64), (K.BLOCK["n_users"], 1))
    als_rank, pop_rank = K.mean_rank(X @ Y.T, tu, ti, hu, hi), K.mean_rank(pop, tu, ti, hu, hi)
    assert als_rank < 8 and pop_rank > 14, (als_rank, pop_rank)          # measured: 6.4 and 15.5


# ---- the recorded distances the GPU tolerances come from ----------------------------------------------------------------
@pytest.mark.parametrize("dim", K.WIDTHS)
def test_fp32_restatement_distances_are_the_recorded_ones(dim):
    for case in [c for c in K.CASES if c[0] == dim]:
        X64, l64 = K.reference(case, "float64")
        X32, l32 = K.reference(case, "float32")
        assert X32.dtype == np.float32 and l32.dtype == np.float32
        dr, dl = float(np.abs(X32 - X64).max()), float(np.abs(l32 - l64).max())
        print(case, "row %.3e loss %.3e" % (dr, dl))
        rec_r, rec_l = K.DEV[case]
        assert 0.95 * rec_r <= dr <= rec_r and 0.95 * rec_l <= dl <= rec_l, (case, dr, dl)
        if case[2] == 0:                                         # no step: the rows bit for bit (but the empty ones: 0)
            empty = np.diff(K.rows(dim)[0]) == 0
            assert X32[~empty].tobytes() == K.rows(dim)[3][~empty].tobytes() and not X32[empty].any()
        assert not X32[0].any() and l32[0] == 0 and not X64[0].any() and l64[0] == 0     # the empty list


def test_no_step_of_a_case_runs_near_the_exit():
    margins = []
    for case in [c for c in K.CASES if c[0] in (32, 256) and c[2] in (3, 8)]:
        Y, G, off, idx, ex, alpha, start, lam, steps = K.case_inputs(case)
        for dt in (np.float64, np.float32):
            R.half_sweep(Y, G, off, idx, ex, alpha, start, lam, steps, dtype=dt, margins=margins)
    assert min(margins) >= R.EXIT_MARGIN                         # (the restatement asserts it on every step anyway)
    print("smallest rs / (RTOL2 rs0) over the executed steps: %.3g" % min(margins))


def test_whole_fit_fp32_distance_is_the_recorded_one():
    X64, Y64, l64 = K.fit_reference("float64")
    X32, Y32, l32 = K.fit_reference("float32")
    got = (float(np.abs(X32 - X64).max()), float(np.abs(Y32 - Y64).max()),
           max(abs(a - b) / abs(a) for a, b in zip(l64, l32)))
    print("fit distances", got)
    for g, rec in zip(got, K.FIT_DEV):
        assert 0.95 * rec <= g <= rec, (got, K.FIT_DEV)
    keep = [t for t in range(1, len(l64)) if (l64[t - 1] - l64[t]) > K.FIT_MIN_DECREASE * l64[t - 1]]
    assert keep == [1, 2, 3]                                      # every half-sweep of the fit decreases by more


def test_dot_chain_restatement_is_the_fused_chain():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(200000).astype(np.float32) for _ in range(3))
    import math
    got = R.fma_exact(a[:2000], b[:2000], c[:2000])
    if hasattr(math, "fma"):
        want = np.array([np.float32(math.fma(float(x), float(y), float(z))) for x, y, z in zip(a[:2000], b[:2000], c[:2000])])
        # math.fma rounds to float64 first: equal unless that is itself a float32 tie
        assert (got == want).mean() > 0.999
    # a constructed tie: 1 + 2^-24 + tiny rounds up only when fused
    one, h = np.float32(1), np.float32(2.0 ** -12)
    x = R.fma_exact(np.array([h]), np.array([h]), np.array([one]))           # 1 + 2^-24: the tie, to even -> 1
    assert x[0] == one
    y = R.fma_exact(np.array([h + np.float32(2.0 ** -30)]), np.array([h]), np.array([one]))   # just above the tie
    assert y[0] == np.nextafter(one, np.float32(2))
    # a tie the fp64 sum lands on from below: 1 + 2^-23 + 2^-24 - 2^-70 must round DOWN to 1 + 2^-23, not to even
    c = np.nextafter(one, np.float32(2))
    z = R.fma_exact(np.array([np.float32(2.0 ** -24) * c]), np.array([np.float32(1 - 2.0 ** -23)]), np.array([c]))
    assert z[0] == c
    Q, Y = rng.standard_normal((3, 32)).astype(np.float32), rng.standard_normal((5, 32)).astype(np.float32)
    out = R.dot_chain(Q, Y)
    assert out.shape == (3, 5) and np.abs(out - Q.astype(np.float64) @ Y.astype(np.float64).T).max() < 1e-5


# ---- the C boundary ---------------------------------------------------------------------------------------------------
def test_size_query_and_argument_rules_need_no_gpu(lib):
    q = lib.anirec_als_gram_workspace_bytes
    assert q(0, 64) == 0 and q(10, 48) == 0 and q(-1, 64) == 0
    assert q(1, 32) == 32 * 32 * 8 and q(_lib.ALS_GRAM_CHUNK, 64) == 64 * 64 * 8
    assert q(_lib.ALS_GRAM_CHUNK + 1, 64) == 2 * 64 * 64 * 8 and q(350000, 256) == 342 * 256 * 256 * 8
    fake = ctypes.c_void_p(4096)                                 # never dereferenced: every call below is refused first
    assert lib.anirec_als_gram(fake, 10, 48, fake, fake, 1 << 30, None) == -1
    assert lib.anirec_als_gram(fake, 0, 64, fake, fake, 1 << 30, None) == -1
    assert lib.anirec_als_gram(None, 10, 64, fake, fake, 1 << 30, None) == -1
    assert lib.anirec_als_gram(fake, 10, 64, fake, ctypes.c_void_p(4100), 1 << 30, None) == -1
    assert lib.anirec_als_gram(fake, 10, 64, fake, fake, 64 * 64 * 8 - 1, None) == -3

    def sweep(dim=64, n_other=10, n_rows=3, lam=0.1, cg=3, alpha=1.0, **null):
        a = dict(Y=fake, G=fake, off=fake, idx=fake, X=fake, loss=fake, err=fake)
        a.update({k: None for k in null})
        return lib.anirec_als_half_sweep(a["Y"], n_other, dim, a["G"], a["off"], a["idx"], None, alpha, None, a["X"],
                                         n_rows, lam, cg, a["loss"], a["err"], None)
    for kw in (dict(dim=48), dict(n_other=0), dict(n_rows=-1), dict(cg=-1), dict(cg=_lib.ALS_MAX_CG + 1),
               dict(lam=-0.1), dict(lam=float("nan")), dict(lam=float("inf")), dict(alpha=-1.0), dict(alpha=float("nan")),
               dict(Y=1), dict(G=1), dict(off=1), dict(X=1), dict(loss=1), dict(err=1)):
        assert sweep(**kw) == -1, kw
    assert sweep(n_rows=0, Y=1, G=1) == 0                        # nothing to do: nothing enqueued
    assert lib.anirec_dot_scores(fake, 3, fake, 0, 64, fake, 10, None) == -1
    assert lib.anirec_dot_scores(fake, 3, fake, 10, 64, fake, 9, None) == -1
    assert lib.anirec_dot_scores(fake, -1, fake, 10, 64, fake, 10, None) == -1
    assert lib.anirec_dot_scores(fake, 3, fake, 10, 48, fake, 10, None) == -1
    assert lib.anirec_dot_scores(None, 3, fake, 10, 64, fake, 10, None) == -1
    assert lib.anirec_dot_scores(None, 0, None, 10, 64, None, 10, None) == 0


def test_python_argument_checks_run_before_any_gpu_use():
    assert ops.check_als(64, 3, 0.01, 1.0) == (64, 3, 0.01, 1.0)
    for f in (48, 0, 512, 64.5, "x"):
        with pytest.raises(ValueError, match="32, 64, 128, 256"):
            ops.check_als(f, 3, 0.01, 1.0)
    for bad in ((64, -1, 0.01, 1.0), (64, 17, 0.01, 1.0), (64, 3, -1.0, 1.0), (64, 3, 0.01, float("nan")),
                (64, 3, float("inf"), 1.0)):
        with pytest.raises(ValueError, match="als"):
            ops.check_als(*bad)
    with pytest.raises(ValueError, match="32, 64, 128, 256"):
        recs.als_fit([0], [0], 1, 1, factors=100)
    with pytest.raises(ValueError, match="index out of range"):
        recs.als_fit([0, 2], [0, 0], 2, 1, factors=32, device="cpu")
    with pytest.raises(ValueError, match="one entry per pair"):
        recs.als_fit([0, 1], [0], 2, 1, factors=32, device="cpu")


# ---- the flag surface ---------------------------------------------------------------------------------------------------
def test_baseline_names_take_als_and_order_it_last():
    assert C.BASELINES == ("popularity", "itemknn") and C.FITTED_BASELINES == ("als",)
    assert C.baseline_names("als") == ("als",) and C.baseline_names(None) == ()
    assert C.baseline_names(["als", "popularity"]) == ("popularity", "als")
    assert C.baseline_names(("als", "itemknn", "als", "popularity")) == ("popularity", "itemknn", "als")
    assert C.baseline_names(["itemknn", "popularity", "itemknn"]) == ("popularity", "itemknn")
    for wrong in ("ALS", "none", ["popularity", "knn"], ""):
        with pytest.raises(ValueError, match="not supported.*popularity, itemknn, als"):
            C.baseline_names(wrong)
    assert C.ALS_DEFAULTS == {"factors": 64, "sweeps": 15, "cg_steps": 3, "alpha": 1.0, "reg": 0.01, "min_rating": 0.0,
                              "seed": 0}


def test_evaluate_als_flags_are_command_line_only():
    mod = load_component("evaluate")
    assert mod.baseline_arg("ALS") == ["als"] and mod.baseline_arg("popularity, als") == ["popularity", "als"]
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    ns = mod.make_cli_parser().parse_args(argv)
    assert {f[len("als_"):]: getattr(ns, f) for f in mod.ALS_FLAGS} == C.ALS_DEFAULTS and ns.baseline == "none"
    ns = mod.make_cli_parser().parse_args(argv + ["--baseline", "als", "--als_factors", "128", "--als_sweeps", "4",
                                                   "--als_cg_steps", "2", "--als_alpha", "40", "--als_reg", "0.1",
                                                   "--als_min_rating", "0.7", "--als_seed", "9"])
    assert (ns.als_factors, ns.als_sweeps, ns.als_cg_steps, ns.als_alpha, ns.als_reg, ns.als_min_rating, ns.als_seed) == \
        (128, 4, 2, 40.0, 0.1, 0.7, 9)
    plain = mod.make_parser().parse_args(argv)
    assert not any(hasattr(plain, f) for f in mod.ALS_FLAGS)
    got = {f[len("itemknn_"):]: getattr(mod.make_cli_parser().parse_args(argv), f) for f in mod.ITEMKNN_FLAGS}
    assert got == C.ITEMKNN_DEFAULTS


def test_evaluate_frame_refuses_bad_als_parameters_before_any_gpu_use(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reached the tables")
    monkeypatch.setattr(C, "_tables_of", boom)
    with pytest.raises(ValueError, match="32, 64, 128, 256"):
        C.evaluate_frame(None, None, 10, [1], 0.5, baseline="als", als={"factors": 100})
    with pytest.raises(ValueError, match="als parameter"):
        C.evaluate_frame(None, None, 10, [1], 0.5, baseline="als", als={"k": 3})
    with pytest.raises(ValueError, match="cg_steps"):
        C.evaluate_frame(None, None, 10, [1], 0.5, baseline=["popularity", "als"], als={"cg_steps": 40})
