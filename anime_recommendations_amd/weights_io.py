"""Model container: the tensors the reference keeps in ``wandb_anime_nn.h5`` under Keras layer
names (``user_embedding`` / ``anime_embedding``: config.yaml:85-86, read back by
similar_anime.py:155,164) stored as safetensors (h5py/TensorFlow are not installable here;
SURVEY.md §8(f)-1 lists .h5 interop as a later row).

Tensor names:  <ID_emb_name>/embeddings, <anime_emb_name>/embeddings, dense/kernel, dense/bias,
batch_normalization/{gamma,beta,moving_mean,moving_variance}; optimiser slots under <optimizer>/ — adam/ (m, v),
rmsprop/ (velocity), adagrad/ (accumulator) or sgd/ (the step count alone).  The file's metadata names the output head
("activation", "loss"); files without them hold the reference's sigmoid + binary_crossentropy model.
"""
from __future__ import annotations

import json

import numpy as np
from safetensors import safe_open
from safetensors.numpy import load_file, save_file

from .schedule import resolve_activation, resolve_loss

HEAD_KEYS = ("w", "b", "gamma", "beta", "mov_mean", "mov_var")
OPTIMIZER_KINDS = ("adam", "sgd", "rmsprop", "adagrad")


def save_model(path, U, A, head, user_ids=None, anime_ids=None, user_name="user_embedding",
               anime_name="anime_embedding", optimizer=None, extra=None, optimizer_name="adam", activation=None,
               loss=None):
    """``optimizer``: the slots of ``optimizer_name`` (TrainEngine.optimizer_state), stored under <optimizer_name>/.
    ``activation`` / ``loss``: the head the model was trained with (Keras names), recorded in the metadata; the
    activation defaults to head["activation"] when the head carries one."""
    if optimizer_name not in OPTIMIZER_KINDS:
        raise ValueError("optimizer_name must be one of %s (got %r)" % (OPTIMIZER_KINDS, optimizer_name))
    t = {
        user_name + "/embeddings": np.ascontiguousarray(U, np.float32),
        anime_name + "/embeddings": np.ascontiguousarray(A, np.float32),
        "dense/kernel": np.array([[head["w"]]], np.float32),
        "dense/bias": np.array([head["b"]], np.float32),
        "batch_normalization/gamma": np.array([head["gamma"]], np.float32),
        "batch_normalization/beta": np.array([head["beta"]], np.float32),
        "batch_normalization/moving_mean": np.array([head["mov_mean"]], np.float32),
        "batch_normalization/moving_variance": np.array([head["mov_var"]], np.float32),
    }
    if user_ids is not None:
        t["index/user_ids"] = np.ascontiguousarray(user_ids, np.int64)
    if anime_ids is not None:
        t["index/anime_ids"] = np.ascontiguousarray(anime_ids, np.int64)
    for k, v in (optimizer or {}).items():
        t[optimizer_name + "/" + k] = np.ascontiguousarray(v)
    meta = {"format": "anime_recommendations_amd/1", "user_layer": user_name, "anime_layer": anime_name}
    if activation is None:
        activation = head.get("activation")
    if activation is not None:
        meta["activation"] = resolve_activation(activation)
    if loss is not None:
        meta["loss"] = resolve_loss(loss)
    meta.update({k: json.dumps(v) for k, v in (extra or {}).items()})
    save_file(t, path, metadata=meta)
    return path


def load_model(path, user_name="user_embedding", anime_name="anime_embedding"):
    """Returns dict(U, A, head, user_ids, anime_ids, optimizer, optimizer_name, activation, loss): the slots found under
    the first optimiser prefix the file holds and that optimiser's name (None when it holds no slots); the activation
    the file records (sigmoid for files that record none) and its loss (None when it records none).  ``head`` keeps
    the six BatchNorm-folded scalars alone; ``model_head`` adds the activation for the predict calls."""
    t = load_file(path)
    with safe_open(path, framework="np") as f:
        meta = f.metadata() or {}
    ukey, akey = user_name + "/embeddings", anime_name + "/embeddings"
    if ukey not in t or akey not in t:
        raise KeyError("model file %s has no layers %r / %r (has %s)" % (path, user_name, anime_name, sorted(t)))
    head = {"w": float(t["dense/kernel"].reshape(-1)[0]), "b": float(t["dense/bias"][0]),
            "gamma": float(t["batch_normalization/gamma"][0]), "beta": float(t["batch_normalization/beta"][0]),
            "mov_mean": float(t["batch_normalization/moving_mean"][0]),
            "mov_var": float(t["batch_normalization/moving_variance"][0])}
    kind = next((o for o in OPTIMIZER_KINDS if any(k.startswith(o + "/") for k in t)), None)
    slots = {k[len(kind) + 1:]: v for k, v in t.items() if k.startswith(kind + "/")} if kind else {}
    return {"U": t[ukey], "A": t[akey], "head": head, "user_ids": t.get("index/user_ids"),
            "anime_ids": t.get("index/anime_ids"), "optimizer": slots, "optimizer_name": kind,
            "activation": resolve_activation(meta.get("activation", "sigmoid")),
            "loss": resolve_loss(meta["loss"]) if "loss" in meta else None}


def model_head(model):
    """The head dict of a loaded model for ops' predict calls: its scalars and the activation it was trained with."""
    return dict(model["head"], activation=model.get("activation", "sigmoid"))
