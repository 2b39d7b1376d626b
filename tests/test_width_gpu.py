"""GPU tests of the embedding widths 32, 64 and 256 (the *_w entry points): the train step, validation and the exact
serving kernels against the NumPy oracle at each width, the zero-padded 128-wide run as a second yardstick for 32 and
64, determinism, `_w(..., 128)` against the old symbols bit for bit, bad widths at the C boundary, stale workspaces,
and the four components end to end at 64.

Shapes are the smallest at which a width can still go wrong: batches that are no multiple of the 8 / 4 / 2 / 1 rows a
wave holds, the last table row in the batch, rows with far more than ANIREC_CHUNK contributions, more than one
workgroup, k on both sides of ANIREC_MAX_TOPK.  Tolerances are those of the 128-wide tests they mirror (named at each
use); none depends on the width."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import metrics_restatement as mr
import poison
from oracle import anirec_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
WIDTHS = (32, 64, 256)
EINVAL = -1


def _problem(seed, n_u, n_a, n, D, zipf=1.2):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-0.05, 0.05, (n_u, D)).astype(f32)
    A = rng.uniform(-0.05, 0.05, (n_a, D)).astype(f32)
    ui = rng.integers(0, n_u, n).astype(np.int64)
    ai = ((rng.zipf(zipf, n) - 1) % n_a).astype(np.int64)
    t = (rng.integers(0, 11, n) / 10).astype(f32)
    return U, A, ui, ai, t


def _engine(U, A, B, arena=8, head_w=1.2, **kw):
    from anime_recommendations_amd.engine import TrainEngine
    eng = TrainEngine(U.shape[0], A.shape[0], max_batch=B, arena_steps=arena, width=U.shape[1], **kw)
    eng.set_head(w=head_w)
    eng.set_weights(U, A)
    eng.reset_optimizer()
    return eng


def _epoch(eng, ui, ai, t, B, lr):
    from anime_recommendations_amd import schedule
    n = len(ui)
    starts = np.arange(0, n, B)
    counts = np.minimum(B, n - starts)
    eng.set_epoch(ui, ai, t, starts, counts, schedule.step_rates(eng.optimizer, lr, 1, len(starts)))
    return starts, counts


def _snapshot(eng):
    eng.synchronize()
    return dict(W=eng.W.cpu().numpy().copy(), M=eng.M.cpu().numpy().copy(), V=eng.V.cpu().numpy().copy(),
                rec=eng.read_state())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. forward and head -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_forward_and_head_match_oracle(D):
    """test_train_gpu.test_forward_and_head_match_oracle at B = 37 (no multiple of the rows a wave holds at any
    width), the last row of each table in the batch; its tolerances"""
    from anime_recommendations_amd.engine import read_ws
    n_u, n_a, B = 300, 70, 37
    U, A, ui, ai, t = _problem(2, n_u, n_a, B, D)
    ui[-1], ai[-1] = n_u - 1, n_a - 1
    eng = _engine(U, A, B)
    assert eng.width == D and not eng.lazy and tuple(eng.W.shape) == (n_u + n_a, D)
    eng.set_epoch(ui, ai, t, [0], [B], [orc.adam_alpha(1e-5, 1)])
    eng.fwd()
    head = orc.new_head(w=1.2)
    f, g, met = orc.grads(U, A, ui, ai, t, head)
    eng.synchronize()
    pk = eng.packets.cpu().numpy()
    pc = (B + 3) & ~3
    np.testing.assert_allclose(pk[:B], f["c"], atol=3e-7)
    np.testing.assert_array_equal(pk[pc:pc + B], t)
    assert pk[2 * pc:2 * pc + 1].view(np.int32)[0] == B
    np.testing.assert_allclose(read_ws(eng, "su")[:B], f["su"], rtol=1e-6)
    np.testing.assert_allclose(read_ws(eng, "sa")[:B], f["sa"], rtol=1e-6)
    eng.head()
    dy = read_ws(eng, "dy")[:B]
    dy_o = (f["p"] - t) / f32(B)
    np.testing.assert_allclose(dy, dy_o, atol=np.abs(dy_o).max() * 2e-5)
    hp = read_ws(eng, "hpart")[:8].astype(np.float64)          # one head workgroup
    zh = (f["z"] - f["mu"]) * f["r"]
    assert abs(hp[0] - float(np.sum(dy_o, dtype=np.float64))) < 1e-7
    assert abs(hp[1] - float(np.sum(dy_o.astype(np.float64) * zh))) < 1e-7
    assert abs(hp[2] / B - float(met["bce"])) < 2e-6
    assert abs(hp[3] / B - float(met["mse"])) < 1e-6
    eng.prep(0, 1)
    eng.bwd()
    eng.adam()
    rec = eng.read_state()
    assert abs(rec["bn_mu"] - f["mu"]) < 1e-6 and abs(rec["bn_var"] - f["var"]) < 1e-7
    assert abs(rec["last_loss"] - met["loss"]) < 2e-6 and abs(rec["last_mse"] - met["mse"]) < 1e-6
    assert abs(rec["reg_sumsq"] - met["reg"]) / met["reg"] < 1e-6
    assert rec["step_fwd"] == 1 and rec["step_bwd"] == 0
    eng.close()


# ---- 2. train steps vs the NumPy oracle ----------------------------------------------------------------------------
SMALL, SKEWED = (300, 200, 256, 1, 1.3), (2000, 64, 4096, 3, 1.05)
STEP_CASES = [(SMALL, "adam", "binary_crossentropy", "sigmoid"), (SKEWED, "adam", "binary_crossentropy", "sigmoid"),
              (SMALL, "sgd", "binary_crossentropy", "sigmoid"), (SMALL, "rmsprop", "binary_crossentropy", "sigmoid"),
              (SMALL, "adagrad", "binary_crossentropy", "sigmoid"), (SMALL, "adam", "mean_squared_error", "linear")]


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("shape,kind,loss,act", STEP_CASES,
                         ids=["%s-%s-%s-B%d" % (k, l[:3], a[:3], s[2]) for s, k, l, a in STEP_CASES])
def test_train_steps_match_oracle(D, shape, kind, loss, act):
    """test_train_gpu.test_train_steps_match_oracle / test_optimizers_gpu.test_engine_run_matches_the_restated_update
    at each width; their bars.  The second shape has rows with hundreds of contributions (64 anime, zipf 1.05)."""
    from anime_recommendations_amd import ops
    n_u, n_a, B, steps, zipf = shape
    n = B * steps - (B // 3 if steps > 1 else 0)      # ragged last batch
    U, A, ui, ai, t = _problem(3, n_u, n_a, n, D, zipf)
    lr = 3e-5
    st = orc.new_state(U, A, orc.new_head(w=1.2), optimizer=kind)
    eng = _engine(U, A, B, optimizer=kind, loss=loss, activation=act)
    starts, counts = _epoch(eng, ui, ai, t, B, lr)
    mets = [orc.train_step(st, ui[s:s + c], ai[s:s + c], t[s:s + c], lr, loss=loss, activation=act)[0]
            for s, c in zip(starts, counts)]
    eng.run(len(starts), use_graph=False)
    rec = eng.read_state()
    assert rec["step_fwd"] == len(starts)
    tol = lr * 2e-3 * len(starts) + 1e-9
    np.testing.assert_allclose(eng.U.cpu().numpy(), st["U"], atol=tol)
    np.testing.assert_allclose(eng.A.cpu().numpy(), st["A"], atol=tol)
    M, V = eng.M.cpu().numpy(), eng.V.cpu().numpy()
    assert M.shape == V.shape == (n_u + n_a, D)
    if kind == "adam":
        np.testing.assert_allclose(M[:n_u], st["mU"], atol=np.abs(st["mU"]).max() * 1e-4)
        np.testing.assert_allclose(M[n_u:], st["mA"], atol=np.abs(st["mA"]).max() * 1e-4)
    else:
        assert (M == 0).all() and (np.array(rec["adam_m"]) == 0).all()
    if kind != "sgd":
        np.testing.assert_allclose(V[:n_u], st["vU"], atol=np.abs(st["vU"]).max() * 1e-4)
        np.testing.assert_allclose(V[n_u:], st["vA"], atol=np.abs(st["vA"]).max() * 1e-4)
        np.testing.assert_allclose(np.array(rec["adam_v"]), st["head"]["v"], atol=np.abs(st["head"]["v"]).max() * 1e-4)
    else:
        assert (V == 0).all()
    h = st["head"]
    for k in ("w", "gamma", "beta"):
        assert abs(float(rec[k]) - float(h[k])) < tol, k
    assert abs(float(rec["b"]) - float(h["b"])) <= 2.05 * lr * len(starts)
    assert abs(rec["mov_mean"] - h["mov_mean"]) < 1e-6 and abs(rec["mov_var"] - h["mov_var"]) < 1e-6
    assert abs(rec["last_loss"] - mets[-1]["loss"]) < 5e-6
    loss_epoch = sum(float(m["loss"]) * c for m, c in zip(mets, counts)) / n
    assert abs(eng.epoch_metrics()[0] - loss_epoch) < 5e-6
    assert (eng.rowmap.cpu().numpy() == 0).all()
    hd = {k: float(rec[k]) for k in ("w", "b", "gamma", "beta", "mov_mean", "mov_var")}
    p = ops.predict_pairs(eng.U, eng.A, dict(hd, activation=act), ui[:500], ai[:500]).cpu().numpy()
    np.testing.assert_allclose(p, orc.predict_pairs(st["U"], st["A"], h, ui[:500], ai[:500], activation=act), atol=1e-5)
    eng.close()


# ---- 3. the zero-padded 128-wide run -------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 64])
def test_native_width_equals_the_zero_padded_128_run(D):
    """A D-wide table padded with zero columns trains the same model through the 128 path (the pad columns see a zero
    gradient and zero weights).  Native W against W128[:, :D] at the oracle test's tol; the History losses at rtol
    3e-6, test_train_gpu's figure between two GPU paths."""
    n_u, n_a, B, steps = 300, 200, 256, 3
    n = B * steps - B // 3
    U, A, ui, ai, t = _problem(5, n_u, n_a, n, D, 1.3)
    lr = 3e-5

    def run(Ux, Ax, **kw):
        eng = _engine(Ux, Ax, B, **kw)
        _epoch(eng, ui, ai, t, B, lr)
        eng.reset_metrics()
        eng.run(steps, use_graph=False)
        out = _snapshot(eng)
        out["loss"] = eng.epoch_metrics()[0]
        eng.close()
        return out

    pad = lambda X: np.concatenate([X, np.zeros((X.shape[0], 128 - D), f32)], 1)
    nat, ref = run(U, A), run(pad(U), pad(A), lazy=False)
    assert (ref["W"][:, D:] == 0).all() and (ref["M"][:, D:] == 0).all()
    tol = lr * 2e-3 * steps + 1e-9
    assert not np.array_equal(nat["W"][:n_u], U)
    np.testing.assert_allclose(nat["W"], ref["W"][:, :D], atol=tol)
    np.testing.assert_allclose(nat["M"], ref["M"][:, :D], atol=np.abs(ref["M"]).max() * 1e-4)
    np.testing.assert_allclose(nat["V"], ref["V"][:, :D], atol=np.abs(ref["V"]).max() * 1e-4)
    np.testing.assert_allclose(nat["loss"], ref["loss"], rtol=3e-6)
    np.testing.assert_allclose(nat["rec"]["last_loss"], ref["rec"]["last_loss"], rtol=3e-6)


# ---- 4. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_runs_are_bitwise_reproducible_and_graph_equals_eager(D):
    U, A, ui, ai, t = _problem(4, 1500, 300, 9 * 500 - 123, D, 1.1)
    B, lr = 500, 5e-5
    outs = []
    for use_graph in (False, False, True):
        eng = _engine(U, A, B, arena=8)             # graph blocks of 4 steps, 9 steps: two replays and an eager tail
        _epoch(eng, ui, ai, t, B, lr)
        eng.run(9, use_graph=use_graph)
        outs.append(_snapshot(eng))
        eng.close()
    assert np.isfinite(outs[0]["W"]).all() and not np.array_equal(outs[0]["W"][:1500], U)
    for o in outs[1:]:
        for k in ("W", "M", "V"):
            assert np.array_equal(_bits(o[k]), _bits(outs[0][k])), k
        assert o["rec"].tobytes() == outs[0]["rec"].tobytes()


# ---- 5. _w(..., 128) is the old call -------------------------------------------------------------------------------
class _PlainSymbols:
    """An engine's library with every descriptor twin NAME_w(desc, 128, ...) answered by the plain NAME(desc, ...).
    It relies on how TrainEngine calls its library: through ``eng.lib``, with (desc, width) as the first two arguments
    of every ``*_w`` call it makes after the constructor."""

    def __init__(self, lib):
        self._lib, self.called = lib, set()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith("_w"):
            return fn
        plain = getattr(self._lib, name[:-2])

        def call(desc, width, *args):
            assert width == 128
            self.called.add(name[:-2])
            return plain(desc, *args)
        return call


def test_twins_at_128_are_the_old_symbols_bit_for_bit():
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    U, A, ui, ai, t = _problem(6, 900, 250, 3 * 400 - 77, 128, 1.2)
    B, lr = 400, 4e-5
    assert lib.anirec_train_workspace_bytes(B, 8) == lib.anirec_train_workspace_bytes_w(B, 8, 128)
    outs = []
    for plain in (True, False):
        eng = _engine(U, A, B, lazy=False, metrics=1)       # (the engine calls the twins)
        if plain:       # the same run on eng.desc through anirec_train_init_reg, anirec_trainer_create / _set_metrics /
            eng.lib = _PlainSymbols(lib)                    # _run / _destroy and anirec_eval_metrics
        _epoch(eng, ui, ai, t, B, lr)
        eng.reset_metrics()
        eng.run(3, use_graph=False)
        o = _snapshot(eng)
        o["val"] = eng.eval_logs(ui[:300], ai[:300], t[:300])
        outs.append(o)
        eng.close()
        if plain:
            assert eng.lib.called == {"anirec_train_init_reg", "anirec_trainer_create", "anirec_eval_metrics"}
    assert not np.array_equal(outs[0]["W"][:900], U) and outs[0]["rec"]["step_fwd"] == 3
    for k in ("W", "M", "V"):
        assert np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])), k
    assert outs[0]["rec"].tobytes() == outs[1]["rec"].tobytes()
    assert outs[0]["val"] == outs[1]["val"]

    # serving: ops.* is the _w spelling; every op that had a branch against its plain symbol
    n, dev = 1000, "cuda"
    rng = np.random.default_rng(7)
    W = torch.from_numpy(rng.normal(0, 0.05, (n, 128)).astype(f32)).to(dev)
    Uq = torch.from_numpy(rng.normal(0, 0.05, (n, 128)).astype(f32)).to(dev)
    q = torch.tensor([3, 0, n - 1, 500], dtype=torch.int32, device=dev)
    wb = torch.from_numpy((rng.integers(0, 1 << 32, (4, (n + 31) // 32), dtype=np.uint64)
                           & rng.integers(0, 1 << 32, (4, (n + 31) // 32), dtype=np.uint64)).astype(np.uint32)
                          .view(np.int32)).to(dev)         # about a quarter of the anime watched
    head = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
    h, act = ops._head_struct(head), ops._head_act(head)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = _lib.ptr

    def same(got, want):
        torch.cuda.synchronize()
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy()))

    def sentinel(like):
        return torch.full_like(like, -7)

    def bytes_(nb):
        return torch.empty(int(nb), dtype=torch.uint8, device=dev)

    Wh = ops.rownorm(W)
    out = sentinel(Wh)
    assert lib.anirec_rownorm(P(W), n, P(out), st) == 0
    same(out, Wh)
    sc = ops.cosine_scores(Wh, 500)
    out = sentinel(sc)
    assert lib.anirec_cosine_scores(P(Wh), n, 500, P(out), st) == 0
    same(out, sc)
    for k in (10, 130):                                     # both sides of ANIREC_MAX_TOPK
        large = k > _lib.MAX_TOPK
        i0, s0 = ops.cosine_topk(Wh, q, k)
        i1, s1 = sentinel(i0), sentinel(s0)
        ws = bytes_(lib.anirec_topk_large_workspace_bytes(n, 4, k) if large else lib.anirec_topk_workspace_bytes(n, 4))
        fn = lib.anirec_cosine_topk_large if large else lib.anirec_cosine_topk
        assert fn(P(Wh), n, P(q), 4, None, 1, k, P(i1), P(s1), P(ws), ws.numel(), st) == 0
        same(i1, i0)
        same(s1, s0)
        i0, p0 = ops.predict_topk(Uq, W, head, q, k, wb)
        i1, p1 = sentinel(i0), sentinel(p0)
        ws = bytes_(lib.anirec_predict_topk_large_workspace_bytes(n, 4, k) if large
                    else lib.anirec_predict_workspace_bytes(n, 4, 1))
        fn = lib.anirec_predict_topk_large_act if large else lib.anirec_predict_topk_act
        assert fn(P(Uq), P(W), n, P(q), 4, C.byref(h), act, P(wb), k, P(i1), P(p1), P(ws), ws.numel(), st) == 0
        same(i1, i0)
        same(p1, p0)
        assert int(i0.min()) >= 0                           # (full lists: nothing compared is padding alone)
    pu = torch.from_numpy(rng.integers(0, n, 37).astype(np.int32)).to(dev)
    pa = torch.from_numpy(rng.integers(0, n, 37).astype(np.int32)).to(dev)
    p0 = ops.predict_pairs(Uq, W, head, pu, pa)
    p1 = sentinel(p0)
    assert lib.anirec_predict_pairs_act(P(Uq), P(W), P(pu), P(pa), 37, C.byref(h), act, P(p1), st) == 0
    same(p1, p0)
    g0 = ops.predict_grid(Uq, W, head, q)
    g1 = sentinel(g0)
    ws = bytes_(lib.anirec_predict_workspace_bytes(n, 4, 0))
    assert lib.anirec_predict_grid_act(P(Uq), P(W), n, P(q), 4, C.byref(h), act, P(g1), P(ws), ws.numel(), st) == 0
    same(g1, g0)


# ---- 6. evaluate and eval_logs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("loss,act,mask", [("binary_crossentropy", "sigmoid", 127), ("log_cosh", "softplus", 63)])
def test_evaluate_and_eval_logs_match_oracle(D, loss, act, mask):
    """test_train_gpu.test_evaluate_matches_oracle and test_metrics_gpu.test_eval_metrics_match_the_restatement at
    each width (n = 1001: no multiple of the ratings a workgroup takes); their bars"""
    U, A, ui, ai, t = _problem(13, 700, 150, 1001, D)
    hv = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
    from anime_recommendations_amd.engine import TrainEngine
    eng = TrainEngine(700, 150, max_batch=512, arena_steps=4, loss=loss, activation=act, metrics=mask, width=D)
    eng.set_head(**hv)
    eng.set_weights(U, A)
    st = orc.new_state(U, A, orc.new_head(**hv))
    vl, vm = eng.evaluate(ui, ai, t)
    ev = orc.evaluate(st, ui, ai, t, loss=loss, activation=act)
    assert abs(vl - float(ev["val_loss"])) < 3e-6 and abs(vm - float(ev["val_mse"])) < 1e-6
    logs = eng.eval_logs(ui, ai, t)
    acc, rec = eng.read_metric_acc("val"), eng.read_state()
    want = mr.evaluate(st, ui, ai, t, act, loss)
    assert rec["val_n"] == len(t)
    for k, kind in enumerate(mr.KINDS):
        got, w = float(acc["sum"][k]), want.sum[kind]
        if not mask & (1 << k):
            assert got == 0.0
        elif kind == "accuracy":
            assert abs(got - w) <= want.near_half
        else:
            assert abs(got - w) <= 1e-5 * abs(w) + 1e-6, (kind, got, w)
    if mask & 64:
        assert int(acc["auc_pos"].sum()) + int(acc["auc_neg"].sum()) == len(t) * mr.ONE
        assert int(acc["auc_pos"].sum()) == int(want.pos.sum())
        assert abs(logs["auc"] - want.values()["auc"]) < 1e-5
    assert abs(logs["loss"] - vl) <= 1e-12 * abs(vl) and abs(logs["mse"] - vm) <= 1e-12 * vm
    eng.close()


# ---- 7. rownorm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_rownorm_within_2ulp_of_numpy_and_nan_on_zero_rows(D):
    """the bar of test_reference_fixtures at 128; 1003 rows: several workgroups and a last one that is not full"""
    from anime_recommendations_amd import ops
    W = np.random.default_rng(D).normal(0, 0.05, (1003, D)).astype(f32)
    W[17] = 0
    W[1002] = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        want = W / np.linalg.norm(W, axis=1).reshape(-1, 1)
    got = ops.rownorm(torch.from_numpy(W)).cpu().numpy()
    assert got.shape == W.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[17]).all() and np.isnan(got[1002]).all()
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 2 * np.spacing(np.abs(want[ok]).astype(f32)))


# ---- 8. cosine -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_cosine_scores_are_the_k_ordered_fma_chain(D):
    """test_infer_gpu.test_cosine_scores_are_the_defined_fma_chain_bitwise at each width: equal to
    oracle.dot_chain_f32 bit for bit but for the NumPy emulation's rare double-rounded ties (its own bar: 0.1 % of
    the rows, 1.2e-7 there).  At 256 the chain runs through two LDS slices."""
    from anime_recommendations_amd import ops
    W = np.random.default_rng(1).normal(0, 0.05, (777, D)).astype(f32)
    Wh = ops.rownorm(torch.from_numpy(W))
    Whn = Wh.cpu().numpy()
    for q in (5, 776):
        s = ops.cosine_scores(Wh, q).cpu().numpy()
        ref = orc.dot_chain_f32(Whn, Whn[q])
        assert (s == ref).mean() > 0.999
        np.testing.assert_allclose(s, ref, atol=1.2e-7)
    # the tile kernel (more than 16 queries) runs the same chain: bitwise equal to the few-query kernel
    qs = list(range(0, 40))
    i_many, s_many = ops.cosine_topk(Wh, qs, 5, exclude_self=False)
    for j in (0, 17, 39):
        i_few, s_few = ops.cosine_topk(Wh, [qs[j]], 5, exclude_self=False)
        assert torch.equal(i_many[j], i_few[0]) and np.array_equal(_bits(s_many[j].cpu().numpy()), _bits(s_few[0].cpu().numpy()))


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("k", [10, 200])
def test_cosine_topk_equals_the_oracle_lists(D, k):
    """n = 1000, a keep mask, exclude_self, two duplicated rows (a tie must resolve to the ascending index); k = 200
    is above ANIREC_MAX_TOPK (anirec_cosine_topk_large_w).  The lists equal oracle.cosine_topk on the oracle's own
    chain wherever its top k + 1 scores are apart by more than the emulation's rounding, and the oracle's selection
    on the GPU's scores always (test_infer_gpu.test_cosine_topk_indices_exact)."""
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(2)
    n = 1000
    W = rng.normal(0, 0.05, (n, D)).astype(f32)
    W[11] = W[4]
    W[12] = W[4]
    keep = rng.random(n) < 0.7
    keep[[4, 11, 12]] = True
    Wh = ops.rownorm(torch.from_numpy(W))
    Whn = Wh.cpu().numpy()
    queries = [4, 0, n - 1, 11] + list(rng.integers(0, n, 4))
    idx, sim = ops.cosine_topk(Wh, queries, k, exclude_self=True, keep=keep.astype(np.uint8))
    idx, sim = idx.cpu().numpy(), sim.cpu().numpy()
    oi_all, os_all = orc.cosine_topk(Whn, queries, k, exclude_self=True, mask=keep)
    for j, q in enumerate(queries):
        s = ops.cosine_scores(Wh, q).cpu().numpy()
        oi, os_ = orc.topk_desc(s, k, exclude=q, mask=keep)
        assert (idx[j, :len(oi)] == oi).all() and (sim[j, :len(oi)] == os_).all(), (j, q)
        assert (idx[j, len(oi):] == -1).all()
        ref = orc.dot_chain_f32(Whn, Whn[q])
        if np.array_equal(ref, s):
            assert (idx[j] == oi_all[j]).all() and np.array_equal(_bits(sim[j]), _bits(os_all[j]))
    assert idx[0][0] == 11 and idx[0][1] == 12        # ties -> ascending index (the query, row 4, is excluded)


# ---- 9. predict ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_predict_grid_and_topk_match_oracle(D, act):
    """test_infer_gpu.test_predict_pairs_grid_topk_match_oracle on 70 users x 1000 anime (the tile kernel: more than
    16 queries, neither count a multiple of the 64 x 64 tile) with blocked bits, k = 10 and k = 200"""
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(4)
    n_u, n_a = 300, 1000
    U = rng.normal(0, 0.05, (n_u, D)).astype(f32)
    A = rng.normal(0, 0.05, (n_a, D)).astype(f32)
    head = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
    oh = orc.new_head(**head)
    hd = dict(head, activation=act)
    tU, tA = torch.from_numpy(U).cuda(), torch.from_numpy(A).cuda()
    users = [n_u - 1, 0] + list(rng.integers(0, n_u, 68))
    G = ops.predict_grid(tU, tA, hd, users).cpu().numpy()
    np.testing.assert_allclose(G, orc.predict_grid(U, A, oh, users, activation=act), atol=1e-5)      # BASELINE bar
    ui, ai = rng.integers(0, n_u, 777), rng.integers(0, n_a, 777)
    ui[-1], ai[-1] = n_u - 1, n_a - 1
    p = ops.predict_pairs(tU, tA, hd, ui, ai).cpu().numpy()
    np.testing.assert_allclose(p, orc.predict_pairs(U, A, oh, ui, ai, activation=act), atol=1e-5)
    watched = rng.random((len(users), n_a)) < 0.3
    bits = np.zeros((len(users), (n_a + 31) // 32), np.uint32)
    for j in range(len(users)):
        for a in np.nonzero(watched[j])[0]:
            bits[j, a >> 5] |= np.uint32(1) << np.uint32(a & 31)
    for k in (10, 200):
        ti, tp = ops.predict_topk(tU, tA, hd, users, k, bits.view(np.int32))
        ti, tp = ti.cpu().numpy(), tp.cpu().numpy()
        for j in range(len(users)):
            oi, op = orc.topk_desc(G[j], k, mask=~watched[j])
            assert (ti[j] == oi).all() and (tp[j] == op).all(), (k, j)
    # a few users take the GEMV-shaped kernel: the same ratings bit for bit
    G3 = ops.predict_grid(tU, tA, hd, users[:3]).cpu().numpy()
    assert np.array_equal(_bits(G3), _bits(G[:3]))


# ---- 10. bad widths at the C boundary ------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 48, 512])
def test_bad_width_is_einval_and_writes_nothing(bad):
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    dev = "cuda"
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, k, nq = 64, 5, 3
    W = torch.randn(n, 512, device=dev)              # (wide enough for whatever a wrong kernel would read)
    q = torch.tensor([1, 2, 3], dtype=torch.int32, device=dev)
    head = _lib.Head(1.0, 0.0, 1.0, 0.0, 0.0, 1.0)
    PAT = 0x5A

    def pat(*shape, dtype=torch.float32):
        return poison.fill(torch.empty(*shape, dtype=dtype, device=dev), PAT)

    outs = []

    def call(fn, *args, out):
        assert fn(*args) == EINVAL, fn.__name__
        outs.extend(out)

    o = pat(n, 512)
    call(lib.anirec_rownorm_w, _lib.ptr(W), n, bad, _lib.ptr(o), st, out=[o])
    o = pat(n)
    call(lib.anirec_cosine_scores_w, _lib.ptr(W), n, bad, 1, _lib.ptr(o), st, out=[o])
    for fn, nb in ((lib.anirec_cosine_topk_w, lib.anirec_topk_workspace_bytes(n, nq)),
                   (lib.anirec_cosine_topk_large_w, lib.anirec_topk_large_workspace_bytes(n, nq, k))):
        oi, os_, ws = pat(nq, k, dtype=torch.int32), pat(nq, k), pat(int(nb), dtype=torch.uint8)
        call(fn, _lib.ptr(W), n, bad, _lib.ptr(q), nq, None, 1, k, _lib.ptr(oi), _lib.ptr(os_), _lib.ptr(ws),
             ws.numel(), st, out=[oi, os_, ws])
    o = pat(nq)
    call(lib.anirec_predict_pairs_w, _lib.ptr(W), _lib.ptr(W), bad, _lib.ptr(q), _lib.ptr(q), nq, C.byref(head), 0,
         _lib.ptr(o), st, out=[o])
    o, ws = pat(nq, n), pat(1 << 20, dtype=torch.uint8)
    call(lib.anirec_predict_grid_w, _lib.ptr(W), _lib.ptr(W), bad, n, _lib.ptr(q), nq, C.byref(head), 0, _lib.ptr(o),
         _lib.ptr(ws), ws.numel(), st, out=[o, ws])
    for fn in (lib.anirec_predict_topk_w, lib.anirec_predict_topk_large_w):
        oi, op, ws = pat(nq, k, dtype=torch.int32), pat(nq, k), pat(16 << 20, dtype=torch.uint8)
        call(fn, _lib.ptr(W), _lib.ptr(W), bad, n, _lib.ptr(q), nq, C.byref(head), 0, None, k, _lib.ptr(oi),
             _lib.ptr(op), _lib.ptr(ws), ws.numel(), st, out=[oi, op, ws])
    assert lib.anirec_predict_workspace_bytes_w(n, nq, 1, bad) == 0
    assert lib.anirec_train_workspace_bytes_w(256, 4, bad) == 0
    # training: a valid 64-wide engine, its descriptor handed to every twin with the bad width
    U, A, ui, ai, t = _problem(8, 50, 20, 64, 64)
    eng = _engine(U, A, 64, arena=4)
    eng.set_epoch(ui, ai, t, [0], [64], [orc.adam_alpha(1e-5, 1)])
    eng.synchronize()
    torch.cuda.synchronize()
    before = [x.clone() for x in (eng._W, eng._M, eng._V, eng.packets, eng.workspace, eng.state_buf, eng.rowmap)]
    d, sp = C.byref(eng.desc), eng._sp()
    assert lib.anirec_train_init_reg_w(d, bad, sp) == EINVAL
    assert lib.anirec_train_prep_w(d, bad, 0, 1, sp) == EINVAL
    for fn in (lib.anirec_train_fwd_w, lib.anirec_train_head_w, lib.anirec_train_bwd_w, lib.anirec_train_adam_w):
        assert fn(d, bad, sp) == EINVAL
    h = C.c_void_p()
    assert lib.anirec_trainer_create_w(d, bad, C.byref(h)) == EINVAL and not h.value
    u32, a32, t32 = (torch.as_tensor(x, device=dev) for x in (ui.astype(np.int32), ai.astype(np.int32), t))
    assert lib.anirec_eval_metrics_w(d, bad, 0, None, _lib.ptr(u32), _lib.ptr(a32), _lib.ptr(t32), 64, sp) == EINVAL
    # a supported width that is not the buffers': the workspace (sized for 64) is too small for 256, and a lazy or
    # multi-GPU descriptor is refused at another width than 128
    assert lib.anirec_train_fwd_w(d, 256, sp) == -3
    torch.cuda.synchronize()
    after = (eng._W, eng._M, eng._V, eng.packets, eng.workspace, eng.state_buf, eng.rowmap)
    for x, y in zip(before, after):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for x in outs:
        assert bool((x.view(torch.uint8) == PAT).all())
    eng.close()


def test_engine_refuses_lazy_and_multi_gpu_at_another_width():
    from anime_recommendations_amd import _lib
    from anime_recommendations_amd.engine import TrainEngine
    with pytest.raises(ValueError, match="lazy"):
        TrainEngine(9000, 100, max_batch=100, arena_steps=4, width=64, lazy=True)
    with pytest.raises(ValueError, match="multi-GPU"):
        TrainEngine(100, 100, max_batch=100, arena_steps=4, width=64, dense_mode=1, n_seg=2)
    with pytest.raises(ValueError, match="32, 64, 128, 256"):
        TrainEngine(100, 100, max_batch=100, arena_steps=4, width=96)
    big = TrainEngine(9000, 100, max_batch=100, arena_steps=4, width=64)       # tables of 90 batches: lazy at 128
    assert big.lazy is False and TrainEngine(9000, 100, max_batch=100, arena_steps=4).lazy is True
    # the C boundary says the same of a descriptor that asks for the lazy update
    lib = _lib.load()
    d = big.desc
    d.lazy, d.lazy_state = 1, d.workspace
    assert lib.anirec_train_fwd_w(C.byref(d), 64, big._sp()) == EINVAL
    d.lazy, d.lazy_state = 0, None
    with pytest.raises(_lib.AnirecError, match="128"):
        big.stage_ticks(True)
    big.close()


# ---- 11. stale workspaces ------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_stale_workspace_bytes_at_64():
    """The training workspace is documented 'zero before FIRST use': afterwards it holds the leftovers of earlier
    steps.  A run on an engine that has just trained another, larger-batch problem (chunk partials, sorted batches and
    head partials of that problem still in the workspace; the packets poisoned on top) equals the run on a fresh
    engine; so does a top-k call whose workspace and outputs held 0x7F / 0xFF bytes."""
    from anime_recommendations_amd import ops
    D, B, lr = 64, 512, 4e-5
    U, A, ui, ai, t = _problem(9, 800, 90, 3 * B - 100, D, 1.1)
    U2, A2, ui2, ai2, t2 = _problem(10, 800, 90, 2 * B, D, 1.02)

    def run(eng):
        eng.set_head(w=1.2)
        eng.set_weights(U, A)
        eng.reset_optimizer()
        _epoch(eng, ui, ai, t, B, lr)
        eng.reset_metrics()
        eng.run(3, use_graph=False)
        return _snapshot(eng)

    fresh = _engine(U, A, B, arena=4)
    want = run(fresh)
    fresh.close()
    stale = _engine(U2, A2, B, arena=4)
    _epoch(stale, ui2, ai2, t2, B, lr)
    stale.run(2, use_graph=False)
    stale.synchronize()
    poison.fill(stale.packets, 0x7F)
    torch.cuda.synchronize()
    got = run(stale)
    stale.close()
    for k in ("W", "M", "V"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert got["rec"].tobytes() == want["rec"].tobytes()
    # serving
    Wh = ops.rownorm(torch.from_numpy(np.random.default_rng(11).normal(0, 0.05, (5000, D)).astype(f32)))
    q = [7, 0, 4999]
    base = {}
    for byte in poison.ORDER:
        for k in (10, 200):
            log = []
            with poison.poisoned(byte, log):
                i, s = ops.cosine_topk(Wh, q, k)
            torch.cuda.synchronize()
            assert sum(log) >= 2 * len(q) * k * 4
            i, s = i.cpu().numpy(), s.cpu().numpy()
            if byte == 0:
                base[k] = (i, s)
                oi, _ = orc.topk_desc(ops.cosine_scores(Wh, 7).cpu().numpy(), k, exclude=7)
                assert (i[0] == oi).all()
            assert np.array_equal(i, base[k][0]) and np.array_equal(_bits(s), _bits(base[k][1])), (byte, k)


# ---- 12. the components end to end at 64 ---------------------------------------------------------------------------
def _run(comp, flags, cwd, env):
    argv = [sys.executable, os.path.join(ROOT, comp, comp + ".py")]
    for k, v in flags.items():
        argv += ["--" + k, str(v)]
    r = subprocess.run(argv, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return r.stdout.decode()


def test_components_end_to_end_at_64(tmp_path, monkeypatch):
    """tests/test_components_gpu.py's pipeline with --embedding_size 64: neural_network, then similar_anime,
    similar_users and model_recs off its model file, each CSV against the oracle on the saved [n, 64] tables"""
    from anime_recommendations_amd import artifacts, components as Cm, data, weights_io
    work = tmp_path
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(work / "store"), ANIREC_SEED="3")
    monkeypatch.setenv("ANIREC_ARTIFACT_DIR", env["ANIREC_ARTIFACT_DIR"])
    paths = data.write_synthetic_dataset(str(work / "data"), n_users=300, n_anime=500, n_ratings=40_000, seed=2)
    artifacts.log_artifact("user_stats.parquet", paths["user_stats"], "parquet")
    artifacts.log_artifact("all_anime.csv", paths["all_anime"], "raw_data")
    artifacts.log_artifact("synopses.csv", paths["synopses"], "raw_data")
    nn = dict(test_size=2000, TPU_INIT=False, embedding_size=64, kernel_initializer="he_normal",
              activation_function="sigmoid", model_loss="binary_crossentropy", optimizer="Adam",
              start_lr=1e-4, min_lr=1e-4, max_lr=5e-4, batch_size=2000, rampup_epochs=2, sustain_epochs=0,
              exp_decay=0.8, weights_artifact="wandb_main_weights.h5", save_weights_only=True,
              checkpoint_metric="val_loss", save_freq="epoch", mode="min", save_best_weights=True, verbose=1,
              epochs=3, save_model=True, model_name="./wandb_anime_nn.h5",
              input_data="user_stats.parquet:latest", project_name="anime_recommendations",
              model_artifact="wandb_anime_nn.h5", history_csv="wandb_anime_nn_history.csv",
              ID_emb_name="user_embedding", anime_emb_name="anime_embedding", merged_name="dot_product",
              main_df_type="parquet", model_type="h5", history_type="history_csv", weights_type="h5",
              model_metrics='["mse"]', l2_reg_factor=1e-4)
    _run("neural_network", nn, str(work), env)
    hist = pd.read_csv(work / "wandb_anime_nn_history.csv")
    assert len(hist) == 3 and np.isfinite(hist.to_numpy()).all() and hist["loss"].iloc[-1] < hist["loss"].iloc[0]
    assert np.allclose(hist["lr"], [f32(x) for x in (1e-4, 3e-4, 5e-4)])
    m = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest"))
    df = pd.read_parquet(paths["user_stats"])
    assert m["U"].shape == (df.user_id.nunique(), 64) and m["A"].shape == (df.anime_id.nunique(), 64)
    assert m["optimizer"]["user_embedding/m"].shape == m["U"].shape
    # the History's val columns: the oracle's evaluation of the saved weights on the hold-out (the component test's
    # check and bars)
    table = data.encode_frame(df)
    _, te = table.split(2000)
    st = dict(U=m["U"], A=m["A"], head=orc.new_head(**m["head"]))
    ev = orc.evaluate(st, table.user[te], table.anime[te], table.rating[te].astype(f32))
    assert abs(float(ev["val_loss"]) - hist["val_loss"].iloc[-1]) < 2e-5
    assert abs(float(ev["val_mse"]) - hist["val_mse"].iloc[-1]) < 1e-5
    common = dict(project_name="anime_recommendations", model="wandb_anime_nn.h5:latest", model_type="h5",
                  main_df="user_stats.parquet:latest", main_df_type="parquet", anime_df="all_anime.csv:latest",
                  anime_df_type="raw_data", ID_emb_name="user_embedding", anime_emb_name="anime_embedding")
    # similar_anime
    anime = pd.read_csv(paths["all_anime"])
    query = anime["Name"].iloc[17]
    _run("similar_anime", dict(common, sypnopsis_df_type="raw_data", sypnopses_df="synopses.csv:latest",
                               anime_query=query, a_query_number=10, random_anime=False,
                               anime_rec_genres='[None, "Action", "Comedy"]', an_spec_genres=True,
                               types='["TV", "Movie"]', spec_types=True, a_rec_type="csv", save_sim_anime=True),
         str(work), env)
    out = pd.read_csv(work / (Cm.clean(query) + ".csv"))
    Wh = orc.rownorm(m["A"])
    ids = np.asarray(m["anime_ids"])
    q = int(np.nonzero(ids == anime["MAL_ID"].iloc[17])[0][0])
    meta = anime.set_index("MAL_ID").reindex(ids)
    keep = meta["Type"].isin(["TV", "Movie"]).to_numpy() & meta["Genres"].str.contains("Action|Comedy").to_numpy()
    s64 = Wh.astype(np.float64) @ Wh[q].astype(np.float64)
    oi, _ = orc.topk_desc(s64.astype(f32), 10, exclude=q, mask=keep)
    assert len(out) == 10
    if np.abs(np.diff(np.sort(s64[keep])[::-1][:11])).min() > 1e-6:
        assert out["Name"].tolist() == meta["Name"].to_numpy()[oi].tolist()
    np.testing.assert_allclose(out["Similarity"].to_numpy(), s64[oi], atol=2e-6)
    # similar_users
    user = int(df.user_id.unique()[5])
    _run("similar_users", dict(common, sim_user_query=user, id_query_number=10, max_ratings=600,
                               sim_random_user=False, num_faves=3, TV_only=True, sim_users_fn="similar_users.csv",
                               sim_users_type="csv", ID_fn="user_id.csv", ID_type="csv", save_sim_locally=True),
         str(work), env)
    out = pd.read_csv(work / ("User_%d.csv" % user))
    Uh = orc.rownorm(m["U"])
    uids = np.asarray(m["user_ids"])
    uq = int(np.nonzero(uids == user)[0][0])
    s64 = Uh.astype(np.float64) @ Uh[uq].astype(np.float64)
    s64[uq] = -np.inf
    o = np.argsort(-s64, kind="stable")[:10]
    if np.abs(np.diff(s64[np.argsort(-s64, kind="stable")[:11]])).min() > 1e-6:
        assert out["similar_users"].tolist() == uids[o].tolist()
    np.testing.assert_allclose(out["similarity"].to_numpy(), s64[o], atol=2e-6)
    # model_recs
    _run("model_recs", dict(main_df="user_stats.parquet:latest", main_df_type="parquet",
                            project_name="anime_recommendations", anime_df="all_anime.csv:latest",
                            anime_df_type="raw_data", sypnopsis_df="synopses.csv:latest", sypnopsis_df_type="raw_data",
                            model="wandb_anime_nn.h5:latest", model_type="h5", model_user_query=user, random_user=False,
                            model_recs_fn="model_recs.csv", save_model_recs=True, model_num_recs=10,
                            anime_types='["TV", "Movie"]', specify_types=True,
                            model_genres='["Action", "Comedy", None]', specify_genres=False, model_ID_flow=True,
                            model_ID_conf=False, model_recs_type="csv", flow_ID="user_id.csv:latest",
                            flow_ID_type="csv"), str(work), env)
    out = pd.read_csv(work / ("User_ID_%d_model_recs.csv" % user))
    watched = set(df[df.user_id == user].anime_id)
    assert len(out) == 10 and not (set(out["anime_id"]) & watched)
    p = orc.predict_pairs(m["U"], m["A"], orc.new_head(**m["head"]), np.full(len(ids), uq), np.arange(len(ids)))
    keep = ~np.isin(ids, list(watched)) & meta["Type"].isin(["TV", "Movie"]).to_numpy()
    oi, op = orc.topk_desc(p, 10, mask=keep)
    np.testing.assert_allclose(out["Prediction"].to_numpy(), op, atol=1e-5)
    if np.abs(np.diff(np.sort(p[keep])[::-1][:11])).min() > 2e-6:
        assert out["anime_id"].tolist() == ids[oi].tolist()
