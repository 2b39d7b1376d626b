"""The fp16 MFMA error windows on rows where they bind (GPU).  The planted rows of tests/mfma_restatement.py put a true
neighbour M about one eps above the window's lower edge (tests/test_mfma_bounds_cpu.py: a window of 0.4 kEpsMfma
loses it); here the kernels must prove every planted row and return the exact path's list and scores, bit for bit.
The rows go to the kernels as built: through ``rownorm`` they would move off the designed fp16 grid."""
import numpy as np
import pytest
import torch

import mfma_restatement as mr
from oracle import anirec_oracle as orc
from oracle import c_oracle

pytestmark = pytest.mark.gpu

KS = (1, 10, 100, 127)


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def _check_cosine(W, Wt, plants, queries, k, idx, sim, fp64=True, overflowed=()):
    """planted rows proven and equal to the exact kernels, the CPU fma chain and (where gaps allow) fp64"""
    idx, sim = idx.cpu().numpy(), sim.cpu().numpy()
    qpos = {int(q): j for j, q in enumerate(queries)}
    ei, es = ops().cosine_topk(Wt, torch.from_numpy(np.asarray(queries, np.int32)).cuda(), k)
    ei, es = ei.cpu().numpy(), es.cpu().numpy()
    proven = idx[:, 0] >= 0
    assert (idx[proven] == ei[proven]).all() and (sim[proven] == es[proven]).all()
    for d in plants:
        j = qpos[d["q"]]
        if d["q"] in overflowed:
            continue
        assert proven[j], d                                   # the window really was exercised, and held
        assert d["M"] in idx[j] and d["O"] not in idx[j]
        oi, os_ = orc.topk_desc(c_oracle.cosine_scores(W, d["q"]), k, exclude=d["q"])
        assert (idx[j] == oi).all() and (sim[j] == os_).all()
        if fp64:
            s64 = W.astype(np.float64) @ W[d["q"]].astype(np.float64)
            s64[d["q"]] = -np.inf
            o64 = np.argsort(-s64, kind="stable")
            gaps = -np.diff(s64[o64[:k + 1]])
            if gaps.min() > 1e-6:
                assert (idx[j] == o64[:k]).all()


def ops():
    from anime_recommendations_amd import ops as o
    return o


def _model_binds(W, plants, k, level=mr.HIGH_LEVEL, users=None):
    """The fixture as built still does what the CPU tests show of the plants: under the model, M and O are the k-th
    and (k+1)-th true neighbours, O's overstated score is tau, and (at the high level) M sits less than 1.2 eps above
    the window's edge — every margin clear of the hardware's accumulation term.  ``users``: model_recs form."""
    lo = 3 * mr.ACC / mr.EPS
    for j, d in enumerate(plants):
        r = mr.plant_report(W, d, k) if users is None else mr.plant_report(W, d, k, qvec=users[j])
        assert r["rank_M"] == k - 1 and r["rank_O"] == k and r["tau_is_O"], (j, r["rank_M"], r["rank_O"])
        assert r["margin_M"] > lo and (level < mr.HIGH_LEVEL or r["margin_M"] < 1.2 - lo), (j, r["margin_M"])


@pytest.mark.parametrize("waves", ["4", "8"])
@pytest.mark.parametrize("k", KS)
def test_planted_cosine_topk_is_proven_and_exact(k, waves, monkeypatch):
    """Anchors and O early in the key stream, every M in the last key tile; both workgroup shapes."""
    monkeypatch.setenv("ANIREC_TOPK_WAVES", waves)
    W, plants = mr.planted_table(k, mr.HIGH_LEVEL, 8, 3000, seed=100 + k)
    _model_binds(W, plants, k)
    Wt = _cuda(W)
    rng = np.random.default_rng(k)
    queries = np.concatenate([[d["q"] for d in plants], rng.integers(0, len(W), 56)]).astype(np.int32)
    idx, sim, _ = ops().cosine_topk_mfma(Wt, queries, k, fallback=False)
    _check_cosine(W, Wt, plants, queries, k, idx, sim)


@pytest.mark.parametrize("level", [0.45, 0.2])
@pytest.mark.parametrize("k", KS)
def test_planted_lower_levels_are_proven_and_exact(k, level):
    """tau truncated in the lower binades of the score"""
    W, plants = mr.planted_table(k, level, 1, 2000, seed=200 + k)
    _model_binds(W, plants, k, level)
    Wt = _cuda(W)
    queries = np.array([plants[0]["q"], 0, len(W) - 1], np.int32)
    idx, sim, _ = ops().cosine_topk_mfma(Wt, queries, k, fallback=False)
    _check_cosine(W, Wt, plants, queries, k, idx, sim)


@pytest.mark.parametrize("splits", [None, "2", "3"])
@pytest.mark.parametrize("k", [10, 127])
def test_planted_few_queries_over_key_range_splits(k, splits, monkeypatch):
    """Eight queries against 18 000 keys: the key tiles of a super-step are shared between workgroups — the
    heuristic's choice (four splits for one row block) and caps of two and three (other region layouts)."""
    if splits is None:
        monkeypatch.delenv("ANIREC_TOPK_SPLITS", raising=False)
    else:
        monkeypatch.setenv("ANIREC_TOPK_SPLITS", splits)
    W, plants = mr.planted_table(k, mr.HIGH_LEVEL, 8, 18_000, seed=300 + k)
    _model_binds(W, plants, k)
    Wt = _cuda(W)
    queries = np.array([d["q"] for d in plants], np.int32)
    st = {}
    idx, sim, nfb = ops().cosine_topk_mfma(Wt, queries, k, fallback=False, stats=st)
    # a split's buffer region (88 entries) can overflow on a plant's 127 anchors at the head of the key stream: such a
    # row is flagged (bit 0, and with it bit 1) and left to the exact path; no other row may come out unproven
    flags = st.get("flag_rows", {})
    assert flags.get(2, 0) == flags.get(1, 0) == nfb and nfb <= (2 if k > 100 else 0)
    over = {int(q) for q, i0 in zip(queries, idx[:, 0].cpu().numpy()) if i0 < 0}
    _check_cosine(W, Wt, plants, queries, k, idx, sim, overflowed=over)


def test_planted_rows_through_the_allpairs_inbox():
    """Every row a query (50 000 rows, a learnt prior, the all-pairs schedule).  Fillers fill the learning batch; every
    plant's M, anchors and O lie in the first main batch and every query in the last.  The last batch streams only the
    learning batch's key tiles and its own: each planted pair reaches its query through the inbox that the first main
    batch's all-pairs launches filled (k_scatter_log -> k_merge_inbox / the re-rank's fold).  No planted query may be
    among the rows re-run without the prior (that path bypasses the all-pairs schedule)."""
    k = 40                                       # (k <= 32 plans no learning batch)
    W, plants = mr.planted_table(k, mr.HIGH_LEVEL, 8, 50_000 - 8 * (k + 2), seed=400, lead=16384)
    assert len(W) == 50_000
    _model_binds(W, plants, k)
    Wt = _cuda(W)
    n = len(W)
    st = {}
    idx, sim, nfb = ops().cosine_topk_mfma(Wt, torch.arange(n, dtype=torch.int32, device="cuda"), k, batch=16384,
                                           allpairs=True, fallback=False, stats=st)
    assert st["allpairs"] is True and st["learn_batches"] == 1 and st["batches"] >= 4
    starts = st["starts"]
    for d in plants:
        keys = d["anchors"] + [d["M"], d["O"]]
        assert starts[1] <= min(keys) and max(keys) < starts[2]          # the first main batch
        assert d["q"] >= starts[-2]                                      # the last batch
    rerun = set(st["rerun_at"].cpu().tolist()) if "rerun_at" in st else set()
    assert not rerun & {d["q"] for d in plants}
    assert st["rerun_rows"] <= 0.02 * n and nfb == 0
    probe = np.unique(np.concatenate([[d["q"] for d in plants], [d["M"] for d in plants], np.arange(0, n, 997)]))
    _check_cosine(W, Wt, plants, probe.astype(np.int32), k, idx[torch.from_numpy(probe).cuda()],
                  sim[torch.from_numpy(probe).cuda()], fp64=False)


def test_unnorm_edge_rows():
    """A planted query at |sum x^2 - 1| = 0.9e-3 is proven; one row at 1.1e-3 sends every query to the exact path."""
    k = 10
    W, plants = mr.planted_table(k, mr.HIGH_LEVEL, 8, 3000, seed=500)
    queries = np.array([d["q"] for d in plants], np.int32)
    qi, fi = plants[0]["q"], max(d["q"] for d in plants) + 1          # a planted query, a filler row
    for target, flagged in ((1 + 0.9e-3, False), (1 + 1.1e-3, True), (1 - 0.9e-3, False), (1 - 1.1e-3, True)):
        V = W.copy()
        if target > 1:     # the query through its free component (its designed ones stay put)
            V[qi] = mr.with_sumsq(V[qi], target, plants[0]["q_free"])
        else:
            V[fi] = (V[fi] * np.sqrt(target / np.sum(V[fi].astype(np.float64) ** 2))).astype(np.float32)
        assert mr.unnorm_flag(V) == flagged
        if not flagged:
            _model_binds(V, plants, k)
        Vt = _cuda(V)
        st = {}
        idx, sim, nfb = ops().cosine_topk_mfma(Vt, queries, k, fallback=False, stats=st)
        if flagged:
            assert nfb == len(queries) and st["flag_rows"][4] == len(queries)
            assert (idx.cpu().numpy() == -1).all()
            idx, sim, _ = ops().cosine_topk_mfma(Vt, queries, k)          # the exact path answers
            ei, es = ops().cosine_topk(Vt, queries, k)
            assert torch.equal(idx, ei) and torch.equal(sim, es)
        else:
            assert nfb == 0
            _check_cosine(V, Vt, plants, queries, k, idx, sim, fp64=False)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("w", [1.7, -1.7])
@pytest.mark.parametrize("act", mr.ACTS)
def test_planted_predict_topk_is_proven_and_exact(act, w, masked):
    """model_recs: the same plants as user and anime rows (a negative folded slope screens with the user rows
    negated: the users are stored as -q so that the fp16 operand is the designed one)."""
    k = 10
    U, A, plants = mr.predict_split(*mr.planted_table(k, mr.HIGH_LEVEL, 8, 3000, seed=600))
    _model_binds(A, plants, k, users=U)
    head = dict(w=w, b=0.1, gamma=1.0, beta=0.3, mov_mean=0.0, mov_var=1.0, activation=act)
    hs, _ = mr.head_fold(head)
    sign = -1.0 if hs < 0 else 1.0
    Ut, At = _cuda(U * np.float32(sign)), _cuda(A)
    users = np.arange(len(U), dtype=np.int32)
    bits = None
    if masked:                                   # a third of the fillers watched; no plant's own rows
        rng = np.random.default_rng(7)
        own = {a for d in plants for a in d["anchors"] + [d["M"], d["O"]]}
        wat = (rng.random((len(U), len(A))) < 0.3)
        wat[:, sorted(own)] = False
        bits = np.zeros((len(U), (len(A) + 31) // 32), np.uint32)
        for a in np.flatnonzero(wat.any(0)):
            bits[:, a >> 5] |= wat[:, a].astype(np.uint32) << np.uint32(a & 31)
        bits = bits.view(np.int32)
    mi, mp, nfb = ops().predict_topk_mfma(Ut, At, head, users, k, bits, fallback=False)
    ei, ep = ops().predict_topk(Ut, At, head, users, k, bits)
    mi, mp, ei, ep = (x.cpu().numpy() for x in (mi, mp, ei, ep))
    assert nfb == 0
    assert (mi == ei).all() and (mp == ep).all()
    for j, d in enumerate(plants):
        assert d["M"] in mi[j] and d["O"] not in mi[j]


# ---------------------------------------------------------------------------------------------------------------
# predict grid: split-fp16 MFMA against an fp64 evaluation of the head
# ---------------------------------------------------------------------------------------------------------------
def _adversarial_rows(rng):
    n = 128
    rows = []
    ramp = 1 + 1e-3 * np.arange(n) / n
    rows.append(ramp / np.linalg.norm(ramp))                           # coherent: every product the same sign
    v = 256 / np.sqrt(n)
    g = float(np.float16(v))
    x = np.full(n, (g + 0.49 * mr._up(g)) / 256)                        # hi residual at its largest, same sign
    rows.append(x / np.linalg.norm(x))
    x = np.full(n, (g + 2e-5) / 256)                                   # lo an fp16 subnormal (2e-5 < 6.1e-5)
    rows.append(x / np.linalg.norm(x))
    x = 1e-3 * rng.normal(0, 1, n)
    x[3] = 1.0                                                          # one dominant component
    rows.append(x / np.linalg.norm(x))
    rows.append(rng.normal(0, 1, n) * 1e-8)                             # sum x^2 ~ 1e-14: under the 1e-12 clamp
    rows.append(np.zeros(n))                                            # zero row: cosine 0
    rows.append(mr.subnormal_row(rng))
    base = np.stack(rows)
    out = np.concatenate([base, -base, rng.normal(0, 0.05, (25, n))]).astype(np.float32)
    return out


def _fp64_grid(U, A, hs, hb, act):
    def nrm(X):
        X = X.astype(np.float64)
        return X / np.sqrt(np.maximum((X * X).sum(1), 1e-12))[:, None]
    u, a = nrm(U), nrm(A)
    c = u @ a.T
    S = np.abs(u) @ np.abs(a).T
    return c, S, mr.act64(act, hs * c + hb)


def _derived_bar(act, hs, hb, c, S, r):
    """The bar anirec_predict_mfma.hip's precision statement gives, term by term.
    Cosine (relative to S = sum |u_k a_k| of the normalised rows):
      split: |v - hi - lo| <= 2^-22 |v| per operand, the dropped lo*lo <= 2^-22 |u_k a_k|      3 x 2^-22
      accumulation: 8 K-steps x 3 MFMAs x 16 products, each add charged one fp32 rounding       384 x 2^-24
        (no finer internal precision of the MFMA's sums is documented)
      normalisation in fp32: sum of squares, sqrt, divide, scale (<= 66 roundings per row)      134 x 2^-24
      lo in the fp16 subnormals: 2^-25 per component, / 2^8                                     ~ 2^-30
    Head: y = c hs + hb in fp32 (two roundings of |c hs| + |hb| + |y|, with hs, hb folded in fp32).
    Activation: error in y times max act' (sigmoid 1/4, others 1), plus the fast forms' own error — sigmoid exp2 and
    rcp within 1 ulp each (4 ulps of r in all), tanh / softplus 1e-6 absolute (the kernel's statement), linear / relu
    one rounding — plus the rounding of the fp32 output."""
    e_c = S * (3 * 2.0 ** -22 + (384 + 134) * 2.0 ** -24) + 2.0 ** -30
    y = hs * c + hb
    e_y = abs(hs) * e_c + 2.0 ** -23 * (np.abs(hs * c) + abs(hb) + np.abs(y))
    slope = 0.25 if act == "sigmoid" else 1.0
    own = {"sigmoid": 4 * 2.0 ** -24 * np.abs(r), "tanh": 1e-6, "softplus": 1e-6}.get(act, 0.0)
    return slope * e_y + own + 2.0 ** -24 * np.abs(r)


SUITE_HEADS = [dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4),
               dict(w=-2.0, b=0.3, gamma=1.1, beta=0.1, mov_mean=-0.02, mov_var=0.9)]


@pytest.mark.parametrize("act", mr.ACTS)
def test_predict_grid_mfma_on_adversarial_rows_within_the_derived_bar(act):
    rng = np.random.default_rng(77)
    U = _adversarial_rows(rng)
    A = np.concatenate([_adversarial_rows(rng), rng.normal(0, 0.05, (300, 128)).astype(np.float32)])
    Ut, At = _cuda(U), _cuda(A)
    users = np.arange(len(U), dtype=np.int32)
    worst = 0.0
    for i, h in enumerate(SUITE_HEADS + [dict(w=12.0, b=0.0, gamma=1.0, beta=0.2, mov_mean=0.0, mov_var=1.0)]):
        head = dict(h, activation=act)
        hs, hb = mr.head_fold(head)
        G = ops().predict_grid_mfma(Ut, At, head, users).cpu().numpy().astype(np.float64)
        c, S, ref = _fp64_grid(U, A, hs, hb, act)
        bar = _derived_bar(act, hs, hb, c, S, ref)
        err = np.abs(G - ref)
        assert (err <= bar).all(), (act, h, float(err.max()), float(bar[np.unravel_index(np.argmax(err - bar), bar.shape)]))
        worst = max(worst, float(err.max()))
        if i < len(SUITE_HEADS):                  # the documented contract against the fp32 path on the suite's heads
            Gf = ops().predict_grid(Ut, At, head, users).cpu().numpy()
            np.testing.assert_allclose(G, Gf, atol=1e-5, rtol=0)
    print("predict_grid_mfma %s: worst |err| against fp64 %.3g" % (act, worst))
