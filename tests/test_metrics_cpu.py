"""CPU tests of --model_metrics: the metric resolver, the AUC assembly from bins against Keras' threshold definition,
trainer.fit's History columns, monitor and restore with a CPU stand-in engine, and the new C ABI entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import metrics_restatement as mr
from anime_recommendations_amd import _lib, data, schedule, trainer
from oracle import anirec_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the resolver ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names,want", [
    (["mse"], [("mse", "mse")]),
    (["MSE", "Mean_Absolute_Error"], [("MSE", "mse"), ("Mean_Absolute_Error", "mae")]),
    (("mape", "msle", "log_cosh"), [("mape", "mape"), ("msle", "msle"), ("log_cosh", "logcosh")]),
    (["logcosh", "ce"], [("logcosh", "logcosh"), ("ce", "bce")]),
    (["crossentropy"], [("crossentropy", "bce")]),
    (["binary_crossentropy", "acc"], [("binary_crossentropy", "bce"), ("acc", "accuracy")]),
    (["BCE", "binary_accuracy"], [("BCE", "bce"), ("binary_accuracy", "accuracy")]),
    (["mae", "accuracy", "AUC", "RootMeanSquaredError"],
     [("mae", "mae"), ("accuracy", "accuracy"), ("auc", "auc"), ("root_mean_squared_error", "rmse")]),
    (["auc", "rootmeansquarederror"], [("auc", "auc"), ("root_mean_squared_error", "rmse")]),
    ([], []),
])
def test_resolver_keys_kinds_and_order(names, want):
    assert schedule.resolve_metrics(names) == want


def test_resolver_mask():
    r = schedule.resolve_metrics(["mse", "RootMeanSquaredError"])
    assert schedule.metric_mask(r) == 0
    r = schedule.resolve_metrics(["mae", "mape", "msle", "logcosh", "bce", "accuracy", "AUC"])
    assert schedule.metric_mask(r) == 127
    assert schedule.metric_mask(schedule.resolve_metrics(["AUC"])) == _lib.METRIC_AUC


@pytest.mark.parametrize("bad", [["mse", "mean_squared_error"], ["acc", "accuracy"], ["precision"], ["Recall"],
                                 ["mse", 3], "mse", '["mse"]', None, ["cosine_similarity"]])
def test_resolver_refuses_with_the_supported_list(bad):
    with pytest.raises(ValueError) as e:
        schedule.resolve_metrics(bad)
    if not isinstance(bad, list) or len(set(bad)) == len(bad) and bad not in (["mse", "mean_squared_error"],
                                                                               ["acc", "accuracy"]):
        assert "supported" in str(e.value)


@pytest.mark.parametrize("act", ["linear", "tanh", "relu", "softplus"])
def test_auc_needs_the_sigmoid_head(act):
    with pytest.raises(ValueError, match="sigmoid"):
        schedule.resolve_metrics(["mae", "AUC"], act)
    assert schedule.resolve_metrics(["mae", "accuracy"], act) == [("mae", "mae"), ("accuracy", "accuracy")]


def test_literal_eval_of_the_flag_strings():
    import ast
    assert schedule.resolve_metrics(ast.literal_eval('["mse"]')) == [("mse", "mse")]
    assert schedule.resolve_metrics(ast.literal_eval('[]')) == []
    assert schedule.resolve_metrics(ast.literal_eval("('mae', 'AUC')")) == [("mae", "mae"), ("auc", "auc")]


# ---- AUC -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bucket_auc_equals_the_threshold_loop_on_hard_labels(seed):
    rng = np.random.default_rng(seed)
    n = 5000
    t = (rng.random(n) < 0.4).astype(np.float32)
    p = np.clip(rng.normal(0.35 + 0.3 * t, 0.2), 0, 1).astype(np.float32)
    p[:10] = [0, 1, 0.5, 1 / 199 + 1e-4, 198 / 199 - 1e-4, 0.25, 0.75, 1e-9, 1 - 1e-7, 0.1]
    pos, neg = mr.auc_bins(p, t)
    assert int(pos.sum()) == int(t.sum()) * mr.ONE and int(pos.sum() + neg.sum()) == n * mr.ONE
    a = mr.auc_from_bins(pos, neg)
    assert abs(a - mr.auc_threshold_loop(p, t)) < 1e-12
    assert 0.5 < a < 1.0
    assert schedule.auc_from_bins(pos, neg) == a          # the host assembly of the engines is the restatement's


def test_auc_soft_labels_and_degenerate_bins():
    p = np.array([0.2, 0.8, 0.6], np.float32)
    t = np.array([0.3, 0.9, 0.5], np.float32)
    pos, neg = mr.auc_bins(p, t)
    assert pos[int(np.ceil(np.float32(0.8) * np.float32(199))) - 1] == round(0.9 * mr.ONE)
    assert abs(mr.auc_from_bins(pos, neg) - mr.auc_threshold_loop(p, t)) < 1e-6
    z = np.zeros(200, np.uint64)
    assert schedule.auc_from_bins(z, z) == 0.0


def test_metric_values_from_sums():
    sums = np.array([2.0, 300.0, 0.5, 0.25, 7.0, 3.0])
    v = schedule.metric_values(127, sums, np.zeros(200), np.zeros(200), 4, 1.0)
    assert v["mae"] == 0.5 and v["mape"] == 75.0 and v["accuracy"] == 0.75 and v["bce"] == 1.75
    assert v["mse"] == 0.25 and v["rmse"] == 0.5
    v = schedule.metric_values(_lib.METRIC_MAE, sums, None, None, 4, 1.0)
    assert set(v) == {"mse", "rmse", "mae"}


# ---- trainer.fit with a CPU stand-in engine --------------------------------------------------------------------
class _MetricEngine:
    """Test double with TrainEngine's metric interface: the oracle trains, the metric columns follow a scripted
    val_auc that peaks at epoch 1"""

    VAL_AUC = [0.60, 0.80, 0.70, 0.65, 0.62, 0.61, 0.60, 0.59]

    def __init__(self, n_u, n_a, l2, metrics):
        import torch
        self.device = torch.device("cpu")
        self.l2, self.metrics = l2, metrics
        self.epoch = -1
        self.steps = 0
        self.calls = []

    def set_head(self, w=1.0, **kw):
        self.w0 = w

    def set_weights(self, U, A):
        self.state = orc.new_state(np.asarray(U), np.asarray(A), orc.new_head(w=self.w0))

    def reset_optimizer(self):
        pass

    def set_epoch(self, u, a, t, starts, counts, alphas):
        self.ep = (np.asarray(u), np.asarray(a), np.asarray(t), starts, counts, alphas)

    def reset_metrics(self):
        self.epoch += 1

    def run(self, n_steps, use_graph=True):
        u, a, t, starts, counts, alphas = self.ep
        for s, c, al in zip(starts, counts, alphas):
            f, g, met = orc.grads(self.state["U"], self.state["A"], u[s:s + c], a[s:s + c], t[s:s + c],
                                  self.state["head"], self.l2)
            orc.adam_update(self.state["A"], self.state["mA"], self.state["vA"], g["A"], al)
            self.steps += 1

    def epoch_metrics(self):
        self.calls.append("epoch_metrics")
        return 0.5, 0.1

    def evaluate(self, u, a, t):
        self.calls.append("evaluate")
        return 0.5, 0.1

    def epoch_logs(self):
        self.calls.append("epoch_logs")
        e = self.epoch
        return {"loss": 1.0 - 0.1 * e, "mse": 0.1, "rmse": 0.1 ** 0.5, "mae": 0.3 - 0.01 * e, "auc": 0.7 + 0.01 * e}

    def eval_logs(self, u, a, t):
        self.calls.append("eval_logs")
        e = self.epoch
        return {"loss": 1.1 - 0.1 * e, "mse": 0.2, "rmse": 0.2 ** 0.5, "mae": 0.4, "auc": self.VAL_AUC[e]}

    def read_state(self):
        return {"w": float(self.epoch), "b": 0.0, "gamma": 1.0, "beta": 0.0, "mov_mean": 0.0, "mov_var": 1.0}

    def synchronize(self):
        pass

    @property
    def U(self):
        import torch
        return torch.from_numpy(self.state["U"] + self.epoch)

    @property
    def A(self):
        import torch
        return torch.from_numpy(self.state["A"] + self.epoch)


def _fit_setup(monkeypatch):
    from anime_recommendations_amd import ops
    monkeypatch.setattr(ops, "gather_ratings", lambda u, a, t, perm: (u[perm], a[perm], t[perm]))
    return data.encode_frame(data.synth_user_stats(n_users=40, n_anime=60, n_ratings=1500, seed=3))


def test_fit_columns_monitor_val_auc_max_and_restore(monkeypatch):
    table = _fit_setup(monkeypatch)
    cfg = trainer.FitConfig(epochs=8, batch_size=256, test_size=200, verbose=1, seed=5, metrics=("mae", "AUC"),
                            monitor="val_auc", mode="max", patience=3)
    mask = schedule.metric_mask(schedule.resolve_metrics(cfg.metrics))
    eng = _MetricEngine(table.n_users, table.n_anime, cfg.l2_reg_factor, mask)
    lines = []
    res = trainer.fit(table, cfg, engine=eng, log=lines.append)
    h = res.history
    cols = ["loss", "mae", "auc", "val_loss", "val_mae", "val_auc", "lr"]
    assert list(h) == cols and list(trainer.history_frame(h).columns) == cols
    assert res.best_epoch == 1 == int(np.argmax(h["val_auc"]))
    assert res.stopped_epoch == 4 and len(h["val_auc"]) == 5
    assert h["val_auc"] == _MetricEngine.VAL_AUC[:5]
    assert h["auc"] == [0.7 + 0.01 * e for e in range(5)]
    # the best epoch's snapshot is restored (the stand-in's tables carry their epoch)
    assert res.head["w"] == 1.0
    np.testing.assert_array_equal(res.U, res.best_U)
    assert lines[0].startswith("Epoch 1/8 - loss: 1.0000 - mae: 0.3000 - auc: 0.7000 - val_loss: 1.1000 - "
                               "val_mae: 0.4000 - val_auc: 0.6000 - lr: ")
    assert "epoch_metrics" not in eng.calls and "evaluate" not in eng.calls


def test_fit_default_metrics_keep_the_two_sum_calls(monkeypatch):
    table = _fit_setup(monkeypatch)
    cfg = trainer.FitConfig(epochs=2, batch_size=256, test_size=200, verbose=0, seed=5)
    eng = _MetricEngine(table.n_users, table.n_anime, cfg.l2_reg_factor, 0)
    res = trainer.fit(table, cfg, engine=eng)
    assert list(res.history) == ["loss", "mse", "val_loss", "val_mse", "lr"]
    assert eng.calls == ["epoch_metrics", "evaluate"] * 2


@pytest.mark.parametrize("monitor", ["val_auc", "auc", "lr", "val_accuracy", "acc"])
def test_unknown_monitor_raises_before_any_step(monkeypatch, monitor):
    table = _fit_setup(monkeypatch)
    cfg = trainer.FitConfig(epochs=2, batch_size=256, test_size=200, verbose=0, metrics=["mse", "mae"],
                            monitor=monitor)
    eng = _MetricEngine(table.n_users, table.n_anime, cfg.l2_reg_factor, _lib.METRIC_MAE)
    with pytest.raises(ValueError, match="monitor"):
        trainer.fit(table, cfg, engine=eng)
    assert eng.steps == 0 and eng.calls == []


def test_fit_refuses_an_engine_with_another_metric_set(monkeypatch):
    table = _fit_setup(monkeypatch)
    cfg = trainer.FitConfig(epochs=1, batch_size=256, test_size=200, verbose=0, metrics=["mae", "auc"])
    eng = _MetricEngine(table.n_users, table.n_anime, cfg.l2_reg_factor, _lib.METRIC_MAE)
    with pytest.raises(ValueError, match="metrics"):
        trainer.fit(table, cfg, engine=eng)
    assert eng.steps == 0


def test_fit_refuses_auc_on_a_linear_head(monkeypatch):
    table = _fit_setup(monkeypatch)
    cfg = trainer.FitConfig(epochs=1, batch_size=256, test_size=200, verbose=0, metrics=["AUC"], activation="linear")
    with pytest.raises(ValueError, match="sigmoid"):
        trainer.fit(table, cfg, engine=_MetricEngine(1, 1, 1e-4, _lib.METRIC_AUC))


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_metric_abi_declared_and_descriptor_still_176_bytes(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anirec.h"
int main(void){
  printf("%d %zu %zu %zu %zu %d %d %d %d %d %d %d %d %u\n", ANIREC_ABI_VERSION, sizeof(anirec_train_desc),
         sizeof(anirec_metric_acc), offsetof(anirec_metric_acc, auc_pos), offsetof(anirec_metric_acc, auc_neg),
         ANIREC_METRIC_MAE, ANIREC_METRIC_MAPE, ANIREC_METRIC_MSLE, ANIREC_METRIC_LOGCOSH, ANIREC_METRIC_BCE,
         ANIREC_METRIC_ACC, ANIREC_METRIC_AUC, ANIREC_AUC_BINS, ANIREC_AUC_ONE);
  return 0; }
'''
    decl = r'''
#include "anirec.h"
int (*f1)(anirec_trainer *, uint32_t, anirec_metric_acc *) = anirec_trainer_set_metrics;
int (*f2)(anirec_dist_stepper *, uint32_t, anirec_metric_acc *) = anirec_dist_stepper_set_metrics;
int (*f3)(const anirec_train_desc *, uint32_t, anirec_metric_acc *, const int32_t *, const int32_t *, const float *,
          int32_t, void *) = anirec_eval_metrics;
'''
    d = tmp_path / "decl.c"
    d.write_text(decl)        # the prototypes, type-checked
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(d)])
    c = tmp_path / "t.c"
    c.write_text(prog)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert v[0] == 5 == _lib.ABI_VERSION
    assert v[1] == 176 == C.sizeof(_lib.TrainDesc)
    D = _lib.METRIC_ACC_DTYPE
    assert v[2] == D.itemsize and v[3] == D.fields["auc_pos"][1] and v[4] == D.fields["auc_neg"][1]
    assert v[5:12] == [_lib.METRIC_MAE, _lib.METRIC_MAPE, _lib.METRIC_MSLE, _lib.METRIC_LOGCOSH, _lib.METRIC_BCE,
                       _lib.METRIC_ACC, _lib.METRIC_AUC] == [schedule.METRIC_BITS[k] for k in
                                                             ("mae", "mape", "msle", "logcosh", "bce", "accuracy",
                                                              "auc")]
    assert v[12] == _lib.AUC_BINS == mr.BINS and v[13] == _lib.AUC_ONE == mr.ONE
    assert tuple(schedule.METRIC_SUM_KINDS) == mr.KINDS


def test_metric_symbols_are_exported_and_bound():
    from anime_recommendations_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    for n in ("anirec_trainer_set_metrics", "anirec_dist_stepper_set_metrics", "anirec_eval_metrics"):
        assert hasattr(lib, n) and n in _lib.PROTOTYPES
    # a NULL handle / descriptor is refused without a GPU
    assert lib.anirec_trainer_set_metrics(None, 1, None) == -1
    assert lib.anirec_dist_stepper_set_metrics(None, 1, None) == -1
    assert lib.anirec_eval_metrics(None, 1, None, None, None, None, 0, None) == -1
