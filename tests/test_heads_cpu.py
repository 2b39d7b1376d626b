"""CPU tests of the output heads (--model_loss / --activation_function / --kernel_initializer): name resolution, the
oracle's statement of the head kernels (include/anirec.h, ANIREC_LOSS_* / ANIREC_ACT_*; oracle.anirec_oracle.head_terms)
against central differences, the Dense(1) initialisers, the weights file and the descriptor layout."""
import os
import subprocess

import numpy as np
import pytest

from anime_recommendations_amd import _lib, schedule, trainer, weights_io
from oracle.anirec_oracle import EPS, ONE_M_EPS, act_fwd, head_terms, loss_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LOSSES = tuple(schedule.LOSSES)
ACTS = tuple(schedule.ACTIVATIONS)


# ---- name resolution ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,want", [
    ("binary_crossentropy", "binary_crossentropy"), ("BCE", "binary_crossentropy"),
    ("BinaryCrossentropy", "binary_crossentropy"), ("mse", "mean_squared_error"),
    ("Mean_Squared_Error", "mean_squared_error"), ("MeanSquaredError", "mean_squared_error"),
    ("MAE", "mean_absolute_error"), ("MeanAbsoluteError", "mean_absolute_error"), ("Huber", "huber"),
    ("logcosh", "log_cosh"), ("LogCosh", "log_cosh"), ("log_cosh", "log_cosh")])
def test_loss_names_resolve(name, want):
    assert schedule.resolve_loss(name) == want


@pytest.mark.parametrize("name", ["Sigmoid", "LINEAR", "tanh", "ReLU", "softplus"])
def test_activation_names_resolve(name):
    assert schedule.resolve_activation(name) == name.lower()


@pytest.mark.parametrize("name,want", [("he_normal", "he_normal"), ("HeNormal", "he_normal"),
                                       ("GLOROT_UNIFORM", "glorot_uniform"), ("LecunNormal", "lecun_normal"),
                                       ("TruncatedNormal", "truncated_normal"), ("Zeros", "zeros"),
                                       ("random_uniform", "random_uniform"), ("Ones", "ones")])
def test_initializer_names_resolve(name, want):
    assert schedule.resolve_initializer(name) == want


@pytest.mark.parametrize("fn,name", [(schedule.resolve_loss, "kl_divergence"), (schedule.resolve_loss, "hinge"),
                                     (schedule.resolve_activation, "selu"), (schedule.resolve_activation, "gelu"),
                                     (schedule.resolve_activation, "swish"),
                                     (schedule.resolve_initializer, "orthogonal")])
def test_unsupported_names_are_refused_with_the_supported_list(fn, name):
    with pytest.raises(ValueError) as e:
        fn(name)
    msg = str(e.value)
    assert repr(name) in msg and "supported:" in msg


def test_the_component_no_longer_rejects_the_three_flags():
    src = open(os.path.join(ROOT, "neural_network", "neural_network.py")).read()
    assert "only %r" not in src
    for fn in ("resolve_loss(args.model_loss)", "resolve_activation(args.activation_function)",
               "resolve_initializer(args.kernel_initializer)"):
        assert fn in src


# ---- the head terms against central differences ----------------------------------------------------------------
def _away_from_kinks(loss, act, y, t):
    """ratings whose (y, p - t) lie at least 1e-3 from the kinks of the pair's loss and activation"""
    p = act_fwd(act, y, np.float64)
    e = p - t
    ok = np.ones(len(y), bool)
    if act == "relu":
        ok &= np.abs(y) > 1e-3
    if loss in ("mean_absolute_error", "huber"):
        ok &= np.abs(e) > 1e-3
    if loss == "huber":
        ok &= np.abs(np.abs(e) - 1) > 1e-3
    if loss == "binary_crossentropy" and act != "sigmoid":
        ok &= (p > 1e-3) & (p < 1 - 1e-3)
    return ok


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("loss", LOSSES)
def test_dy_is_the_derivative_of_the_restated_loss(loss, act):
    rng = np.random.default_rng(7)
    y = rng.uniform(-3, 3, 4000)
    if act in ("linear", "relu"):
        y = rng.uniform(-0.5, 1.5, 4000)       # p in the range a BCE of probabilities sees
    t = rng.integers(0, 11, 4000) / 10
    keep = _away_from_kinks(loss, act, y, t)
    y, t = y[keep], t[keep]
    assert len(y) > 1000
    _, _, g = head_terms(loss, act, y, t, np.float64)
    h = 1e-6
    lp = head_terms(loss, act, y + h, t, np.float64)[1]
    lm = head_terms(loss, act, y - h, t, np.float64)[1]
    num = (lp - lm) / (2 * h)
    np.testing.assert_allclose(g, num, rtol=1e-5, atol=1e-7)


def test_bce_clip_passes_the_gradient_on_the_closed_interval_only():
    p = np.array([0.0, EPS, f32(0.5), ONE_M_EPS, f32(1.0), f32(1.5)], f32)
    t = np.full(6, f32(0.3))
    l, g = loss_terms("binary_crossentropy", p, t)
    assert g[0] == 0 and g[4] == 0 and g[5] == 0
    assert g[1] != 0 and g[2] != 0 and g[3] != 0
    assert np.isfinite(l).all()


# ---- initialisers ---------------------------------------------------------------------------------------------
def _draws(kind, n=4000):
    return np.array([trainer.init_weights(1, 1, 8, seed, kind)[2] for seed in range(n)])


def test_he_normal_draws_the_bits_it_always_drew():
    for seed in (0, 1, 17, 123):
        rng = np.random.Generator(np.random.PCG64(seed))
        rng.uniform(-0.05, 0.05, (30, 128))
        rng.uniform(-0.05, 0.05, (20, 128))
        std = np.sqrt(2.0 / 1.0) / 0.87962566103423978
        w = rng.normal(0.0, std)
        while abs(w) > 2 * std:
            w = rng.normal(0.0, std)
        U, A, w0 = trainer.init_weights(30, 20, 128, seed)
        assert np.float32(w0).view(np.uint32) == np.float32(w).view(np.uint32)
        assert trainer.init_weights(30, 20, 128, seed, "he_normal")[2] == w0
        assert trainer.init_weights(30, 20, 128, seed, "HeNormal")[2] == w0


@pytest.mark.parametrize("kind,std,cut", [("he_normal", np.sqrt(2) / 0.87962566103423978, 2),
                                          ("glorot_normal", 1 / 0.87962566103423978, 2),
                                          ("lecun_normal", 1 / 0.87962566103423978, 2),
                                          ("truncated_normal", 0.05, 2), ("random_normal", 0.05, None)])
def test_normal_initializers_bounds_and_moments(kind, std, cut):
    w = _draws(kind)
    assert abs(w.mean()) < 0.1 * std
    if cut:
        assert np.abs(w).max() <= cut * std * (1 + 1e-6)
        assert np.abs(w).max() > 1.9 * std
        # a normal cut at 2 sigma keeps 0.8796^2 of its variance (the factor the VarianceScaling stddev divides by)
        assert 0.85 * std < w.std() < 0.91 * std
    else:
        assert 0.95 * std < w.std() < 1.05 * std


@pytest.mark.parametrize("kind,lim", [("he_uniform", np.sqrt(6)), ("glorot_uniform", np.sqrt(3)),
                                      ("lecun_uniform", np.sqrt(3)), ("random_uniform", 0.05)])
def test_uniform_initializers_bounds_and_moments(kind, lim):
    w = _draws(kind)
    assert np.abs(w).max() <= lim * (1 + 1e-6) and np.abs(w).max() > 0.99 * lim
    assert abs(w.mean()) < 0.05 * lim
    assert abs(w.std() - lim / np.sqrt(3)) < 0.03 * lim


def test_constant_initializers_and_the_tables_stay_put():
    U0, A0, _ = trainer.init_weights(30, 20, 128, 5)
    for kind, want in (("zeros", 0.0), ("ones", 1.0)):
        U, A, w = trainer.init_weights(30, 20, 128, 5, kind)
        assert w == want
        assert np.array_equal(U, U0) and np.array_equal(A, A0)
    with pytest.raises(ValueError):
        trainer.init_weights(3, 2, 128, 0, "orthogonal")


# ---- the weights file -----------------------------------------------------------------------------------------
def test_weights_file_records_activation_and_loss(tmp_path):
    rng = np.random.default_rng(0)
    U, A = rng.normal(size=(5, 128)).astype(f32), rng.normal(size=(4, 128)).astype(f32)
    head = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
    p = weights_io.save_model(str(tmp_path / "m.safetensors"), U, A, head, activation="ReLU", loss="MSE")
    m = weights_io.load_model(p)
    assert m["activation"] == "relu" and m["loss"] == "mean_squared_error"
    assert "activation" not in m["head"] and weights_io.model_head(m) == dict(m["head"], activation="relu")
    assert all(abs(m["head"][k] - head[k]) < 1e-7 for k in head)
    # the head's own key is taken when no activation is passed
    p2 = weights_io.save_model(str(tmp_path / "m2.safetensors"), U, A, dict(head, activation="tanh"))
    assert weights_io.load_model(p2)["activation"] == "tanh"
    with pytest.raises(ValueError):
        weights_io.save_model(str(tmp_path / "x.safetensors"), U, A, head, activation="selu")


def test_files_without_a_head_record_load_as_sigmoid(tmp_path):
    from safetensors.numpy import save_file
    U, A = np.ones((2, 128), f32), np.ones((3, 128), f32)
    t = {"user_embedding/embeddings": U, "anime_embedding/embeddings": A,
         "dense/kernel": np.array([[1.0]], f32), "dense/bias": np.array([0.0], f32),
         "batch_normalization/gamma": np.array([1.0], f32), "batch_normalization/beta": np.array([0.0], f32),
         "batch_normalization/moving_mean": np.array([0.0], f32),
         "batch_normalization/moving_variance": np.array([1.0], f32)}
    p = str(tmp_path / "old.safetensors")
    save_file(t, p, metadata={"format": "anime_recommendations_amd/1"})
    m = weights_io.load_model(p)
    assert m["activation"] == "sigmoid" and m["loss"] is None
    assert weights_io.model_head(m)["activation"] == "sigmoid"
    p = weights_io.save_model(str(tmp_path / "new.safetensors"), U, A, {k: 1.0 for k in weights_io.HEAD_KEYS})
    assert weights_io.load_model(p)["activation"] == "sigmoid"


# ---- the descriptor -------------------------------------------------------------------------------------------
def test_desc_keeps_abi_5_layout_and_places_loss_and_activation(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anirec.h"
int main(void){
  printf("%d %zu %zu %zu %zu %zu %zu %d %d\n", ANIREC_ABI_VERSION, sizeof(anirec_train_desc),
         offsetof(anirec_train_desc, n_steps), offsetof(anirec_train_desc, loss), offsetof(anirec_train_desc, packets),
         offsetof(anirec_train_desc, optimizer), offsetof(anirec_train_desc, activation), ANIREC_LOSS_LOGCOSH,
         ANIREC_ACT_SOFTPLUS);
  return 0; }
'''
    c = tmp_path / "t.c"
    c.write_text(prog)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    abi, size, off_n, off_loss, off_pk, off_opt, off_act, llog, asp = (
        int(x) for x in subprocess.check_output([str(exe)]).decode().split())
    import ctypes as C
    D = _lib.TrainDesc
    assert abi == 5 == _lib.ABI_VERSION
    # ABI 5 as the optimizer change left it: 176 bytes, optimizer the last field; loss in the old pad2 slot,
    # activation in the tail padding
    assert size == 176 == C.sizeof(D)
    assert off_loss == off_n + 4 == D.loss.offset and off_loss + 4 == off_pk
    assert off_opt == 168 == D.optimizer.offset and off_act == 172 == D.activation.offset
    assert llog == _lib.LOSS_LOGCOSH == schedule.LOSSES["log_cosh"]
    assert asp == _lib.ACT_SOFTPLUS == schedule.ACTIVATIONS["softplus"]
