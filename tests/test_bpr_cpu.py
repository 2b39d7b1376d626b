"""CPU tests of BPR matrix factorisation: the NumPy restatement (tests/bpr_restatement.py) held to its own
rules (the sampler, the stated sigmoid against the fp64 logistic, the order-freedom of a step, the chained fit) and to
popularity on planted blocks; the header, the build list and the bindings; the names, the flag surfaces and the
ValueErrors that come before any GPU use."""
import os
import re

import numpy as np
import pytest

import bpr_restatement as R
from component_cli import load_component
from test_cooc_cpu import _frames, _model, _table

from anime_recommendations_amd import _lib, build, components as C, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"anirec_bpr_workspace_bytes": 4, "anirec_bpr_sample": 14, "anirec_bpr_steps": 22}
# what the restatement below restates: without these the module does not import, so every test here needs the feature
RESTATED = (ops.bpr_sample, ops.bpr_steps, recs.bpr_fit)


def _lists(n_users=12, n_items=29, seed=0):
    rng = np.random.default_rng(seed)
    lens = [0, 1, n_items - 1, n_items] + list(rng.integers(1, 12, n_users - 4))
    u = np.concatenate([np.full(n, r) for r, n in enumerate(lens)])
    i = np.concatenate([np.sort(rng.choice(n_items, n, replace=False)) for n in lens])
    return R.csr(u, i, n_users, n_items), n_items


# ---- the sampler ------------------------------------------------------------------------------------------------------
def test_sampler_never_draws_a_liked_item_and_drops_what_it_must():
    (off, idx, pu), n_items = _lists()
    trip = R.sample(off, idx, pu, n_items, 500, 8, 3, 0, 6).reshape(-1, 3)
    u, i, j = trip.T
    assert (u >= 0).all() and all(R.in_row(off, idx, a, b) for a, b in zip(u, i))      # the positive is a liked pair
    kept = j >= 0
    assert kept.any() and not any(R.in_row(off, idx, a, b) for a, b in zip(u[kept], j[kept]))
    assert (u == 3).any() and (j[u == 3] == -1).all()            # who likes every item drops every slot
    only = int(np.setdiff1d(np.arange(n_items), idx[off[2]:off[3]])[0])
    assert (u == 2).sum() > 50 and set(j[u == 2].tolist()) == {-1, only}         # all but one: found, or dropped
    # with one try a slot of that user is kept exactly when the first candidate is the one unliked item
    one = R.sample(off, idx, pu, n_items, 500, 1, 3, 0, 6).reshape(-1, 3)
    h = np.concatenate([R.slot_hash(3, t, np.arange(500)) for t in range(6)])
    first = R.pick(R.draw(h, 1), n_items)
    sel = one[:, 0] == 2
    assert np.array_equal(one[sel, 2] >= 0, first[sel] == only)
    # the literal form of a few slots
    for s in (0, 7, 499):
        hs = R.slot_hash(3, 4, [s])
        p = int(R.pick(R.draw(hs, 0), len(idx))[0])
        want_j = -1
        for c in range(1, 9):
            cand = int(R.pick(R.draw(hs, c), n_items)[0])
            if not R.in_row(off, idx, pu[p], cand):
                want_j = cand
                break
        assert R.sample(off, idx, pu, n_items, 500, 8, 3, 4, 1)[0, s].tolist() == [pu[p], idx[p], want_j]


def test_draws_depend_on_seed_step_and_slot_only():
    (off, idx, pu), n_items = _lists()
    whole = R.sample(off, idx, pu, n_items, 300, 8, 9, 2, 5)
    assert np.array_equal(R.sample(off, idx, pu, n_items, 300, 8, 9, 4, 2), whole[2:4])      # a range of its own
    assert np.array_equal(R.sample(off, idx, pu, n_items, 100, 8, 9, 2, 5), whole[:, :100])  # a smaller batch: a prefix
    assert np.array_equal(R.sample(off, idx, pu, n_items, 300, 3, 9, 2, 5)[..., :2], whole[..., :2])
    assert not np.array_equal(R.sample(off, idx, pu, n_items, 300, 8, 10, 2, 5), whole)
    assert int(R.mix32([0])[0]) == 0
    x = 1
    for sh, mul in ((16, 0x7feb352d), (15, 0x846ca68b)):                   # mix32, literally
        x ^= x >> sh
        x = (x * mul) & 0xFFFFFFFF
    assert int(R.mix32([1])[0]) == x ^ (x >> 16)


# ---- the sigmoid ------------------------------------------------------------------------------------------------------
def test_sigmoid_is_within_1e_6_of_the_fp64_logistic_and_monotone():
    x = np.linspace(-30.0, 30.0, 2_000_001).astype(np.float32)
    g = R.sigmoid_neg(x)
    assert g.dtype == np.float32
    err = float(np.abs(g.astype(np.float64) - 1.0 / (1.0 + np.exp(x.astype(np.float64)))).max())
    print("stated sigmoid against the fp64 logistic on [-30, 30]: largest absolute error %.3e" % err)
    assert err <= 1e-6
    assert (np.diff(g) <= 0).all()                               # non-increasing in x^
    out = R.sigmoid_neg(np.array([-1e30, -31.0, 31.0, 1e30, np.nan, -np.inf, np.inf], np.float32))
    assert out[0] == out[1] == out[4] == out[5] == R.sigmoid_neg(np.float32([-30.0]))[0]    # the clamp; a NaN is -30
    assert out[2] == out[3] == out[6] == R.sigmoid_neg(np.float32([30.0]))[0] and 0.0 < out[2] < 1e-12
    assert [c.view(np.uint32) for c in (R.L2E, R.C1, R.C2)] == [0x3FB8AA3B, 0x3F317200, 0x35BFBE8E]
    assert float(R.C1) + float(R.C2) == pytest.approx(np.log(2.0), abs=1e-13)


def test_x_hat_is_the_stated_order():
    rng = np.random.default_rng(0)
    for width in R.WIDTHS:
        x = rng.standard_normal((3, width)).astype(np.float32)
        d = rng.standard_normal((3, width)).astype(np.float32)
        got = R.x_hat(x, d)
        for r in range(3):                                       # lane sums, then the butterfly, literally
            v = [np.float32(np.float32(np.float32(x[r, 4 * l] * d[r, 4 * l] + x[r, 4 * l + 1] * d[r, 4 * l + 1]) +
                                       x[r, 4 * l + 2] * d[r, 4 * l + 2]) + x[r, 4 * l + 3] * d[r, 4 * l + 3])
                 for l in range(width // 4)]
            o = width // 8
            while o >= 1:
                v = [np.float32(v[l] + v[l ^ o]) for l in range(len(v))]
                o //= 2
            assert len({a.tobytes() for a in v}) == 1 and got[r].tobytes() == v[0].tobytes()
        assert abs(float(got[0]) - float(x[0].astype(np.float64) @ d[0].astype(np.float64))) < 1e-4


# ---- one step and the whole fit ---------------------------------------------------------------------------------------
def test_a_step_does_not_depend_on_the_order_of_its_triples():
    (off, idx, pu), n_items = _lists()
    rng = np.random.default_rng(1)
    X = (rng.standard_normal((12, 32)) * 0.5).astype(np.float32)
    Y = (rng.standard_normal((n_items, 32)) * 0.5).astype(np.float32)
    trip = R.sample(off, idx, pu, n_items, 400, 8, 0, 0, 1)[0]
    for bias in (0, 1):
        base = R.step(X, Y, trip, 0.05, 0.01, bias)
        assert base[2][0] + base[2][1] == 400 and base[2][1] > 0 and base[3] == 0
        for order in (np.arange(400)[::-1], rng.permutation(400), rng.permutation(400)):
            got = R.step(X, Y, trip, 0.05, 0.01, bias, order=order)
            assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[2:] == base[2:]
        assert (base[0][:, -1] == X[:, -1]).all() == bool(bias)
    # a row no slot touches keeps its bits; a touched one moves
    touched = np.zeros(12, bool)
    touched[trip[trip[:, 2] >= 0, 0]] = True
    assert not touched[3] and (base[0][~touched] == X[~touched]).all() and (base[0][touched] != X[touched]).any()
    # the update, literally, for one touched row and column
    one = R.sample(off, idx, pu, n_items, 1, 8, 5, 0, 1)[0]
    u, i, j = one[0]
    assert j >= 0
    Xn, Yn, counts, _ = R.step(X, Y, one, 0.05, 0.01, 0)
    d = Y[i] - Y[j]
    g = R.sigmoid_neg(R.x_hat(X[u:u + 1], d[None]))[0]
    term = int(np.rint(np.float64(np.float32(g * d[3])) * 2.0 ** 30))
    grad = np.float32(np.float64(term) * 2.0 ** -30)
    want = np.float32(X[u, 3] + np.float32(np.float32(0.05) * np.float32(grad - np.float32(np.float32(0.01) * X[u, 3]))))
    assert Xn[u, 3].tobytes() == want.tobytes() and counts[0] == 1


def test_a_term_above_2_pow_20_is_flagged_and_adds_nothing():
    X = np.zeros((1, 32), np.float32)
    Y = np.zeros((2, 32), np.float32)
    Y[0, 0], Y[0, 1] = 3e6, 1.0
    Xn, Yn, counts, err = R.step(X, Y, np.array([[0, 0, 1]], np.int32), 1.0, 0.0, 0)
    assert err == R.ERR_DIVERGED and Xn[0, 0] == 0.0 and Xn[0, 1] == 0.5      # g = 1/2 at x^ = 0; the large term dropped


def test_the_fit_is_its_steps_chained_with_step0():
    rng = np.random.default_rng(3)
    like = rng.random((20, 15)) < 0.3
    u, i = np.nonzero(like)
    par = dict(factors=32, epochs=3, batch=50, lr=0.05, reg=0.01, tries=8, bias=True, seed=2)
    X, Y, counts = R.fit(u, i, 20, 15, **par)
    off, idx, pu = R.csr(u, i, 20, 15)
    per = -(-len(idx) // 50)
    Xc, Yc = R.start_tables(20, 15, 32, True, 2)
    assert (Xc[:, -1] == 1).all() and (Yc[:, -1] == 0).all()
    rows = []
    for e in range(3):                                           # an epoch a call; then every step a call
        Xc, Yc, c, err = R.steps(Xc, Yc, off, idx, pu, 50, 8, 2, e * per, per, 0.05, 0.01, 1)
        rows.append(c.sum(0))
        assert err == 0
    assert Xc.tobytes() == X.tobytes() and Yc.tobytes() == Y.tobytes() and np.array_equal(np.array(rows), counts)
    Xs, Ys = R.start_tables(20, 15, 32, True, 2)
    for t in range(3 * per):
        Xs, Ys, _, _ = R.steps(Xs, Ys, off, idx, pu, 50, 8, 2, t, 1, 0.05, 0.01, 1)
    assert Xs.tobytes() == X.tobytes() and Ys.tobytes() == Y.tobytes()
    assert (X[:, -1] == 1).all() and (Y[:, -1] != 0).any()       # the user column stays 1: the items' is a bias
    assert counts.shape == (3, 3) and (counts[:, 0] + counts[:, 1] == per * 50).all()


@pytest.mark.parametrize("data_seed", R.BLOCK_SEEDS)
def test_planted_blocks_bpr_ranks_the_held_out_pairs_above_popularity(data_seed):
    tu, ti, hu, hi = R.block_pairs(data_seed)
    X, Y, counts = R.block_fit(data_seed)
    bpr = R.mean_rank(X.astype(np.float64) @ Y.astype(np.float64).T, tu, ti, hu, hi)
    pop = R.mean_rank(np.tile(np.bincount(ti, minlength=40).astype(np.float64), (80, 1)), tu, ti, hu, hi)
    print("planted blocks, data seed %d: mean held-out rank BPR %.2f, popularity %.2f" % (data_seed, bpr, pop))
    assert bpr < pop
    assert counts[-1, 2] > 0.8 * counts[-1, 0]                   # by the last epoch most sampled pairs are in order


# ---- the header, the build list and the bindings ----------------------------------------------------------------------
def test_header_build_list_and_bindings():
    header = open(os.path.join(ROOT, "include", "anirec.h")).read()
    assert re.search(r"#define\s+ANIREC_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5
    for name, n_args in NEW.items():
        m = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
    assert re.search(r"#define\s+ANIREC_BPR_MAX_TRIES\s+16\b", header) and _lib.BPR_MAX_TRIES == 16
    assert re.search(r"#define\s+ANIREC_BPR_ERR_INDEX\s+1\b", header) and _lib.BPR_ERR_INDEX == 1
    assert re.search(r"#define\s+ANIREC_BPR_ERR_DIVERGED\s+2\b", header) and _lib.BPR_ERR_DIVERGED == 2
    assert "anirec_bpr.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "anirec_bpr.hip"))
    for word in ("0x3FB8AA3B", "0x3F317200", "0x35BFBE8E", "2^30", "2^20"):
        assert word in header                                    # the definition is stated in the header
    src = open(os.path.join(build.CSRC, "anirec_bpr.hip")).read()
    assert "expf" not in src.replace("ldexpf", "") and "fp contract(off)" in src


# ---- names, orderings and flag surfaces -------------------------------------------------------------------------------
def test_names_and_pinned_constants():
    assert recs.PAIRWISE_SYSTEMS == ("bpr",) and C.PAIRWISE_BASELINES == ("bpr",)
    assert C.BPR_DEFAULTS == {"factors": 64, "epochs": 30, "batch": 131072, "lr": 0.05, "reg": 0.01, "tries": 8,
                              "bias": True, "min_rating": 0.0, "seed": 0}
    assert recs.bpr_fit.__defaults__[:8] == (64, 30, 131072, 0.05, 0.01, 8, True, 0)
    assert C.baseline_names("bpr") == ("bpr",)
    assert C.baseline_names(["bpr", "rp3", "ease", "content", "hybrid_tuned", "popularity", "als", "hybrid", "itemknn"]) == \
        ("popularity", "itemknn", "als", "hybrid", "hybrid_tuned", "content", "ease", "rp3", "bpr")
    with pytest.raises(ValueError, match="not supported.*content, ease, rp3, bpr"):
        C.baseline_names("bpr2")
    assert recs.check_hybrid(("model", " BPR"))[0] == ("model", "bpr")
    assert recs.check_hybrid(("bpr", "rp3", "als"))[0] == ("bpr", "rp3", "als")
    # the pinned constants and the three pinned lookup lists are as they were
    assert recs.HYBRID_SYSTEMS == ("model", "popularity", "itemknn", "als") and recs.CONTENT_SYSTEMS == ("content",)
    assert recs.EASE_SYSTEMS == ("ease",) and recs.GRAPH_SYSTEMS == ("rp3",)
    assert C.BASELINES == ("popularity", "itemknn") and C.FITTED_BASELINES == ("als",)
    assert C.FUSED_BASELINES == ("hybrid",) and C.TUNED_BASELINES == ("hybrid_tuned",)
    assert C.CONTENT_BASELINES == ("content",) and C.LINEAR_BASELINES == ("ease",) and C.GRAPH_BASELINES == ("rp3",)
    assert list(C._systems()) == ["model", "popularity", "itemknn", "als", "content"]
    assert list(C._system_table()) == ["model", "popularity", "itemknn", "als", "content", "ease"]
    assert list(C._system_lookup()) == ["model", "popularity", "itemknn", "als", "content", "ease", "rp3"]
    assert list(C._system_layers()) == ["model", "popularity", "itemknn", "als", "content", "ease", "rp3", "bpr"]
    assert C._system_params({}, [])["bpr"] == C.BPR_DEFAULTS
    for doc in (recs.bpr_fit.__doc__, C.evaluate_frame.__doc__):
        assert "not tuned on this data" in " ".join(doc.split())        # the defaults are documented as not tuned


def test_evaluate_bpr_flags_are_command_line_only():
    import yaml
    mod = load_component("evaluate")
    assert list(mod.BPR_FLAGS) == ["bpr_factors", "bpr_epochs", "bpr_batch", "bpr_lr", "bpr_reg", "bpr_tries", "bpr_bias",
                                   "bpr_min_rating", "bpr_seed"]
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    ns = mod.make_cli_parser().parse_args(argv)
    assert mod.bpr_args(ns) == C.BPR_DEFAULTS
    ns = mod.make_cli_parser().parse_args(argv + ["--bpr_factors", "128", "--bpr_epochs", "5", "--bpr_batch", "4096",
                                                  "--bpr_lr", "0.1", "--bpr_reg", "0.02", "--bpr_tries", "3", "--bpr_bias",
                                                  "False", "--bpr_min_rating", "0.6", "--bpr_seed", "7"])
    assert mod.bpr_args(ns) == {"factors": 128, "epochs": 5, "batch": 4096, "lr": 0.1, "reg": 0.02, "tries": 3,
                                "bias": False, "min_rating": 0.6, "seed": 7}
    for bad in (["--bpr_bias", "maybe"], ["--bpr_factors", "6.5"], ["--bpr_lr", "fast"]):
        with pytest.raises(SystemExit):
            mod.make_cli_parser().parse_args(argv + bad)
    plain = mod.make_parser().parse_args(argv)
    assert not any(hasattr(plain, f) for f in mod.BPR_FLAGS) and mod.bpr_args(plain) == {}
    ml = yaml.safe_load(open(os.path.join(ROOT, "evaluate", "MLproject")))
    params = ml["entry_points"]["main"]["parameters"]
    assert not set(params) & set(mod.BPR_FLAGS)
    assert list(params) == mod.STR_FLAGS + ["baseline"] + list(mod.OPTIONAL_FLAGS)      # the MLproject is as it was
    assert list(mod.RP3_FLAGS) == ["rp3_alpha", "rp3_beta", "rp3_neighbours", "rp3_min_rating"]     # and so are these
    assert mod.wants(mod.make_cli_parser().parse_args(argv + ["--baseline", "popularity,bpr"]), "bpr")
    assert mod.wants(mod.make_cli_parser().parse_args(argv + ["--baseline", "hybrid", "--hybrid_systems", "model,bpr"]), "bpr")
    assert not mod.wants(mod.make_cli_parser().parse_args(argv + ["--baseline", "als"]), "bpr")


# ---- ValueErrors before any GPU use -----------------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    """any use of the device fails the test"""
    def boom(*a, **kw):
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(ops, "_need_gpu", boom)
    monkeypatch.setattr(_lib, "call", boom)
    import torch
    monkeypatch.setattr(torch.Tensor, "cuda", boom)


def test_check_bpr(no_gpu):
    assert ops.check_bpr(64, "100", 8, "0.05", 0, True) == (64, 100, 8, 0.05, 0.0, 1)
    assert ops.check_bpr(256, 1, 16, 0.0, 1.0, False)[5] == 0
    with pytest.raises(ValueError, match="32, 64, 128, 256"):
        ops.check_bpr(48, 100, 8, 0.05, 0.01)
    for batch in (0, -5, 2 ** 31):
        with pytest.raises(ValueError, match="batch"):
            ops.check_bpr(64, batch, 8, 0.05, 0.01)
    for tries in (0, 17):
        with pytest.raises(ValueError, match="tries"):
            ops.check_bpr(64, 100, tries, 0.05, 0.01)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            ops.check_bpr(64, 100, 8, bad, 0.01)
        with pytest.raises(ValueError, match="finite"):
            ops.check_bpr(64, 100, 8, 0.05, bad)
    with pytest.raises(ValueError, match="bias"):
        ops.check_bpr(64, 100, 8, 0.05, 0.01, bias=2)


def test_value_errors_come_before_any_gpu_use(no_gpu):
    for kw, match in ((dict(factors=48), "32, 64, 128, 256"), (dict(batch=0), "batch"), (dict(tries=17), "tries"),
                      (dict(lr=-1.0), "finite"), (dict(reg=float("nan")), "finite"), (dict(epochs=-1), "epochs"),
                      (dict(bias="yes"), "bias")):
        with pytest.raises(ValueError, match=match):
            recs.bpr_fit([0, 1], [0, 1], 2, 2, **kw)
    with pytest.raises(ValueError, match="one entry per pair"):
        recs.bpr_fit([0, 1], [0], 2, 2)
    with pytest.raises(ValueError, match="one pair at least"):
        recs.bpr_fit([], [], 2, 2)
    with pytest.raises(ValueError, match="out of range"):
        recs.bpr_fit([0, 2], [0, 1], 2, 2)
    with pytest.raises(ValueError, match="out of range"):
        recs.bpr_fit([0, 1], [0, -1], 2, 2)
    with pytest.raises(ValueError, match="n_users"):
        recs.bpr_fit([0], [0], 0, 2)
    with pytest.raises(ValueError, match="2\\^31 steps"):
        recs.bpr_fit([0, 1, 1], [0, 1, 1], 2, 2, batch=1, epochs=2 ** 30)
    table = _table()
    model = _model(table)
    for par, match in (({"factors": 48}, "32, 64, 128, 256"), ({"tries": 0}, "tries"), ({"lr": float("inf")}, "finite"),
                       ({"epochs": -2}, "epochs"), ({"batch": 0}, "batch"), ({"momentum": 0.9}, "bpr parameter")):
        with pytest.raises(ValueError, match=match):
            C.evaluate_frame(model, table, 200, [1], 0.5, baseline="bpr", bpr=par)
    with pytest.raises(ValueError, match="tries"):                      # as a hybrid member too
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="hybrid", hybrid={"systems": ("model", "bpr")},
                         bpr={"tries": 99})
    ev = load_component("evaluate")
    eargv = []
    for f in ev.STR_FLAGS:
        eargv += ["--" + f, "x"]
    for extra in (["--baseline", "bpr"], ["--baseline", "popularity,hybrid", "--hybrid_systems", "model,bpr"]):
        with pytest.raises(ValueError, match="32, 64, 128, 256"):       # before any file is opened
            ev.go(ev.make_cli_parser().parse_args(eargv + extra + ["--bpr_factors", "100"]))
