"""The train step's moments row by row (tests/train_rows.py's bar) at widths 32, 64, 128 and 256: one step from
initialisation on the batch of run lengths 1 ... 65, with Adam (dense and eager; at 128 also the lazy update, bit for
bit) and with SGD, RMSprop and Adagrad, and at 128 on the first batch of tests/test_sparse_tail_gpu.py's hand-built
epoch (rows of 33 and 64 chunks at the chunk slots' edges).  M and V are held to the fp64 oracle within K times the
fp32 oracle's own row-relative distance from it; W, the head scalars and the loss to tests/test_train_edges_gpu.py's
bars.  Every test prints the kernel's distance in units of the fp32 oracle's (run with -s to see them)."""
import numpy as np
import pytest

import train_rows as tr
from oracle import anirec_oracle as orc
from test_width_gpu import _engine

pytestmark = pytest.mark.gpu
f32 = np.float32
LR = tr.LR
WIDTHS = (32, 64, 128, 256)


def _step(eng, ui, ai, t, rates):
    """one eager step on the whole batch; (W, M, V) on the host and the state record"""
    eng.set_epoch(ui, ai, t, [0], [len(ui)], rates)
    eng.reset_metrics()
    eng.run(1, use_graph=False)
    eng.synchronize()
    rec = eng.read_state()
    assert int(rec["step_fwd"]) == 1
    return eng.W.cpu().numpy(), eng.M.cpu().numpy(), eng.V.cpu().numpy(), rec


def _check_moments(M, V, o64, unit, ui, ai, n_u, longest, what):
    """M and V row by row; the figures printed are kernel / fp32-oracle, each the largest row ratio to the fp64 oracle"""
    got = {"mU": M[:n_u], "mA": M[n_u:], "vU": V[:n_u], "vA": V[n_u:]}
    figures = {}
    try:
        for k, u in unit.items():
            # a bar above a quarter of one contribution among `longest` equal ones could hide a lost one
            assert tr.K * u <= 1.0 / (4 * longest), (k, u)
            tr.check_rows(got[k], o64[k], u, tr.K, k, ui if k[1] == "U" else ai, figures=figures)
    finally:
        print("%s kernel/fp32-oracle %s  unit %s" % (what, "  ".join("%s %.2f" % kv for kv in figures.items()),
                                                     "  ".join("%s %.2e" % kv for kv in unit.items())))
    return figures


def _check_rest(W, rec, o32, met, n_u, eng):
    """W, the head scalars and the loss of one step at tests/test_train_edges_gpu.py's bars; the row map clear"""
    tol = LR * 2e-3 + 1e-9
    assert np.isfinite(W).all()
    np.testing.assert_allclose(W[:n_u], o32["U"], atol=tol)
    np.testing.assert_allclose(W[n_u:], o32["A"], atol=tol)
    h = o32["head"]
    for k in ("w", "gamma", "beta"):
        assert abs(float(rec[k]) - float(h[k])) < tol, k
    assert abs(float(rec["b"]) - float(h["b"])) <= 2.05 * LR
    assert abs(rec["mov_mean"] - h["mov_mean"]) < 1e-6 and abs(rec["mov_var"] - h["mov_var"]) < 1e-6
    assert abs(rec["last_loss"] - met["loss"]) < 5e-6
    assert abs(eng.epoch_metrics()[0] - float(met["loss"])) < 5e-6
    assert (eng.rowmap.cpu().numpy() == 0).all()


@pytest.mark.parametrize("D", WIDTHS)
def test_adam_step_on_the_run_lengths_row_by_row(D):
    (U, A, ui, ai, t), o32, o64, met, unit = tr.reference(D)
    eng = _engine(U, A, tr.N, lazy=False)
    assert eng.width == D and not eng.lazy
    W, M, V, rec = _step(eng, ui, ai, t, [orc.adam_alpha(LR, 1)])
    _check_moments(M, V, o64, unit, ui, ai, tr.N_U, tr.RUNS, "adam D=%d" % D)
    _check_rest(W, rec, o32, met, tr.N_U, eng)
    eng.close()
    if D == 128:        # the lazy update, forced: the same bits
        lz = _engine(U, A, tr.N, lazy=True)
        assert lz.lazy
        Wl, Ml, Vl, _ = _step(lz, ui, ai, t, [orc.adam_alpha(LR, 1)])
        for x, y, what in ((W, Wl, "W"), (M, Ml, "M"), (V, Vl, "V")):
            bad = np.nonzero((x.view(np.uint32) != y.view(np.uint32)).any(1))[0]
            assert not len(bad), "lazy %s differs from dense in rows %s" % (what, bad[:8].tolist())
        assert (lz.rowmap.cpu().numpy() == 0).all()
        lz.close()


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("kind", orc.KINDS)
def test_other_optimizers_on_the_run_lengths_row_by_row(kind, D):
    from anime_recommendations_amd import schedule
    (U, A, ui, ai, t), o32, o64, met, unit = tr.reference(D, kind)
    eng = _engine(U, A, tr.N, optimizer=kind)
    W, M, V, rec = _step(eng, ui, ai, t, schedule.step_rates(kind, LR, 1, 1))
    assert (M == 0).all() and (np.array(rec["adam_m"]) == 0).all()
    if kind == "sgd":
        assert not unit and (V == 0).all() and (np.array(rec["adam_v"]) == 0).all()
    else:
        assert sorted(unit) == ["vA", "vU"]
        _check_moments(M, V, o64, unit, ui, ai, tr.N_U, tr.RUNS, "%s D=%d" % (kind, D))
        hv = o32["head"]["v"]
        np.testing.assert_allclose(np.array(rec["adam_v"]), hv, atol=np.abs(hv).max() * 1e-4)
    _check_rest(W, rec, o32, met, tr.N_U, eng)
    eng.close()


def test_first_step_of_the_heavy_row_epoch_row_by_row():
    """anime row 0 takes all 2048 ratings (64 chunks, the first slots of the grid) and user row 1000 takes 1056 (33
    chunks) beside 992 single ratings: the layout tests/test_sparse_tail_gpu.py builds for the chunk slots' edges, its
    first step held row by row"""
    import test_sparse_tail_gpu as tail
    U, A, ui_all, ai_all, t_all, starts, counts = tail._problem()
    ui, ai, t = tail._batches()[0]
    assert len(ui) == tail.B and tr.run_lengths(ai, tail.N_A)[0] == 2048 and tr.run_lengths(ui, tail.N_U)[1000] == 1056
    o32, met = tr.oracle_step(U, A, ui, ai, t, dtype=f32)
    o64, _ = tr.oracle_step(U, A, ui, ai, t, dtype=np.float64)
    unit = tr.row_unit(o32, o64)
    eng = _engine(U, A, tail.B, lazy=False)
    W, M, V, rec = _step(eng, ui, ai, t, [orc.adam_alpha(LR, 1)])
    _check_moments(M, V, o64, unit, ui, ai, tail.N_U, 2048, "heavy rows D=128")
    _check_rest(W, rec, o32, met, tail.N_U, eng)
    eng.close()
