"""NumPy restatement of the Keras-2.12 SGD / RMSprop / Adagrad rules (include/anirec.h, ANIREC_OPT_*) on the oracle's
gradients (oracle.anirec_oracle.grads): the reference the optimizer kernels are held to, shared by
tests/test_optimizers_gpu.py and tests/test_train_edges_gpu.py."""
import numpy as np

from oracle import anirec_oracle as orc

f32 = np.float32
KINDS = ("sgd", "rmsprop", "adagrad")
SLOT_INIT = {"sgd": 0.0, "rmsprop": 0.0, "adagrad": 0.1}


def opt_update(kind, W, s, g, lr):
    """In place, fp32, in the order the header writes it; s: the RMSprop velocity / Adagrad accumulator."""
    lr = f32(lr)
    if kind == "sgd":
        W[...] = W - g * lr
    elif kind == "rmsprop":
        s[...] = f32(0.9) * s + f32(0.1) * (g * g)
        W[...] = W - (lr * g) * (f32(1) / np.sqrt(s + f32(1e-7)))
    elif kind == "adagrad":
        s[...] = s + g * g
        W[...] = W - (lr * g) / np.sqrt(s + f32(1e-7))
    else:
        raise ValueError(kind)


def new_state(kind, U, A, w=1.2):
    st = orc.new_state(U, A, orc.new_head(w=w))
    st["sU"] = np.full_like(U, SLOT_INIT[kind])
    st["sA"] = np.full_like(A, SLOT_INIT[kind])
    st["head"]["v"] = np.full(4, SLOT_INIT[kind], np.float32)
    return st


def step(kind, st, ui, ai, t, lr, l2=1e-4):
    """orc.train_step with the update rule of `kind` (gradients, moving statistics and metrics unchanged)."""
    head = st["head"]
    f, g, met = orc.grads(st["U"], st["A"], ui, ai, t, head, l2)
    opt_update(kind, st["U"], st["sU"], g["U"], lr)
    opt_update(kind, st["A"], st["sA"], g["A"], lr)
    hp = np.array([head["w"], head["b"], head["gamma"], head["beta"]], f32)
    hg = np.array([g["w"], g["b"], g["gamma"], g["beta"]], f32)
    hv = head["v"].astype(f32)
    opt_update(kind, hp, hv, hg, lr)
    head["w"], head["b"], head["gamma"], head["beta"] = hp
    head["v"] = hv
    dec = f32(1.0 - orc.BN_MOMENTUM)
    head["mov_mean"] = f32(head["mov_mean"]) - (f32(head["mov_mean"]) - f["mu"]) * dec
    head["mov_var"] = f32(head["mov_var"]) - (f32(head["mov_var"]) - f["var"]) * dec
    return met
