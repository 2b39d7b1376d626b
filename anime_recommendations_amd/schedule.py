"""Learning-rate schedule and optimiser step sizes of the training component (host logic).

Mirrors ``lrfn`` (reference neural_network/neural_network.py:109-125) driven by
``LearningRateScheduler`` (:184-186), the bias-corrected step size of the Keras-2.12
Adam the reference compiles with by default (``optimizer='Adam'``, :104), and the name lookup
``model.compile(optimizer=<name>)`` performs for the other optimisers the kernels implement.
"""
from __future__ import annotations

import numpy as np

ADAM_B1 = 0.9
ADAM_B2 = 0.999

# update rules of the HIP train step, by the name tf.keras.optimizers.get resolves (case-insensitively), with the
# value of anirec_train_desc.optimizer (ANIREC_OPT_*); every one with Keras' default hyper-parameters
OPTIMIZERS = {"adam": 0, "sgd": 1, "rmsprop": 2, "adagrad": 3}


def resolve_optimizer(name):
    """Canonical (lower-case) name of a Keras optimizer the kernels implement; ValueError for any other."""
    key = str(name).lower()
    if key not in OPTIMIZERS:
        raise ValueError("optimizer %r is not supported by the HIP train step (supported: %s)"
                         % (name, ", ".join(sorted(OPTIMIZERS))))
    return key


# output heads of the HIP train step: the Keras losses and output activations by canonical name, with the values of
# anirec_train_desc.loss (ANIREC_LOSS_*) and .activation (ANIREC_ACT_*) — include/anirec.h states what each computes
LOSSES = {"binary_crossentropy": 0, "mean_squared_error": 1, "mean_absolute_error": 2, "huber": 3, "log_cosh": 4}
ACTIVATIONS = {"sigmoid": 0, "linear": 1, "tanh": 2, "relu": 3, "softplus": 4}
# Dense(1) kernel initialisers (trainer.init_weights)
INITIALIZERS = ("he_normal", "he_uniform", "glorot_normal", "glorot_uniform", "lecun_normal", "lecun_uniform",
                "random_normal", "random_uniform", "truncated_normal", "zeros", "ones")

# the other names tf.keras.losses.get / initializers.get resolve to the same objects (lower case): aliases and the
# Keras class names
_LOSS_NAMES = {"bce": "binary_crossentropy", "binarycrossentropy": "binary_crossentropy",
               "mse": "mean_squared_error", "meansquarederror": "mean_squared_error",
               "mae": "mean_absolute_error", "meanabsoluteerror": "mean_absolute_error",
               "logcosh": "log_cosh"}
_INIT_NAMES = {"henormal": "he_normal", "heuniform": "he_uniform", "glorotnormal": "glorot_normal",
               "glorotuniform": "glorot_uniform", "lecunnormal": "lecun_normal", "lecununiform": "lecun_uniform",
               "randomnormal": "random_normal", "randomuniform": "random_uniform",
               "truncatednormal": "truncated_normal", "zeros": "zeros", "ones": "ones"}


def _resolve(what, name, known, aliases):
    key = str(name).lower()
    key = aliases.get(key, key)
    if key not in known:
        raise ValueError("%s %r is not supported by the HIP train step (supported: %s)"
                         % (what, name, ", ".join(sorted(known))))
    return key


def resolve_loss(name):
    """Canonical Keras name of a loss the kernels implement (any case; aliases bce / mse / mae / logcosh and the class
    names resolve too); ValueError, listing the supported set, for any other."""
    return _resolve("loss", name, LOSSES, _LOSS_NAMES)


def resolve_activation(name):
    """Canonical name of an output activation the kernels implement (any case); ValueError for any other — selu, gelu
    and swish among them: they are not monotone, which the top-k paths need."""
    return _resolve("activation", name, ACTIVATIONS, {})


def resolve_initializer(name):
    """Canonical Keras name of a Dense kernel initialiser ``trainer.init_weights`` draws (any case, class names too)."""
    return _resolve("kernel_initializer", name, INITIALIZERS, _INIT_NAMES)


def lrfn(epoch, start_lr=1e-5, max_lr=5e-5, min_lr=1e-5, rampup_epochs=5, sustain_epochs=0,
         exp_decay=0.8):
    """Learning rate of ``epoch`` (0-based): linear ramp start->max over ``rampup_epochs``,
    hold for ``sustain_epochs``, then exponential decay towards ``min_lr``."""
    start_lr, max_lr, min_lr, exp_decay = float(start_lr), float(max_lr), float(min_lr), float(exp_decay)
    rampup_epochs, sustain_epochs = int(rampup_epochs), int(sustain_epochs)
    if epoch < rampup_epochs:
        return (max_lr - start_lr) / rampup_epochs * epoch + start_lr
    if epoch < rampup_epochs + sustain_epochs:
        return max_lr
    return (max_lr - min_lr) * exp_decay ** (epoch - rampup_epochs - sustain_epochs) + min_lr


def adam_alpha(lr, t):
    """lr * sqrt(1 - b2^t) / (1 - b1^t) in fp32, t = 1-based optimiser iteration."""
    f = np.float32
    lr, ts = f(lr), f(t)
    b1p = np.power(f(ADAM_B1), ts, dtype=f)
    b2p = np.power(f(ADAM_B2), ts, dtype=f)
    return f(lr * np.sqrt(f(1) - b2p, dtype=f) / (f(1) - b1p))


def adam_alphas(lr, t_first, n):
    """Vector of step sizes for iterations t_first .. t_first+n-1 (fp32)."""
    f = np.float32
    ts = np.arange(t_first, t_first + n, dtype=f)
    b1p = np.power(f(ADAM_B1), ts, dtype=f)
    b2p = np.power(f(ADAM_B2), ts, dtype=f)
    return (f(lr) * np.sqrt(f(1) - b2p, dtype=f) / (f(1) - b1p)).astype(f)


def step_rates(kind, lr, t_first, n):
    """The per-step rate of anirec_step.alpha for iterations t_first .. t_first+n-1 (fp32): Adam's bias-corrected
    step size (``adam_alphas``), float32(lr) for SGD, RMSprop and Adagrad (no bias correction)."""
    kind = resolve_optimizer(kind)
    if kind == "adam":
        return adam_alphas(lr, t_first, n)
    return np.full(int(n), np.float32(lr), dtype=np.float32)


# Keras metrics of model.compile(metrics=...) (neural_network.py:102-104) the GPU accumulates: name (lower case) ->
# (kind, History key or None = the name as written).  Function metrics keep the string as written, metric classes take
# their default snake-case name (Keras 2.12 compile_utils).  MSE and RMSE come from the squared-error sums every step
# keeps already; every other kind has its ANIREC_METRIC_* bit (METRIC_BITS).
_METRIC_NAMES = {
    "mse": ("mse", None), "mean_squared_error": ("mse", None),
    "mae": ("mae", None), "mean_absolute_error": ("mae", None),
    "mape": ("mape", None), "mean_absolute_percentage_error": ("mape", None),
    "msle": ("msle", None), "mean_squared_logarithmic_error": ("msle", None),
    "logcosh": ("logcosh", None), "log_cosh": ("logcosh", None),
    "binary_crossentropy": ("bce", None), "crossentropy": ("bce", None), "ce": ("bce", None), "bce": ("bce", None),
    "accuracy": ("accuracy", None), "acc": ("accuracy", None), "binary_accuracy": ("accuracy", None),
    "rootmeansquarederror": ("rmse", "root_mean_squared_error"),
    "auc": ("auc", "auc"),
}
METRIC_BITS = {"mse": 0, "rmse": 0, "mae": 1, "mape": 2, "msle": 4, "logcosh": 8, "bce": 16, "accuracy": 32, "auc": 64}
# the order of anirec_metric_acc.sum
METRIC_SUM_KINDS = ("mae", "mape", "msle", "logcosh", "bce", "accuracy")


def resolve_metrics(metrics, activation="sigmoid"):
    """The metric set of ``ast.literal_eval(--model_metrics)``: a list or tuple of Keras metric names (any case; the
    aliases and classes the kernels implement, ``_METRIC_NAMES``).  Returns the ordered [(History key, kind)];
    ValueError, listing the supported names, for an unknown entry, a kind named twice, a bare string, or AUC with an
    output activation other than sigmoid (Keras' AUC asserts predictions in [0, 1])."""
    supported = "supported: %s, AUC, RootMeanSquaredError" % ", ".join(
        sorted(k for k, (_, key) in _METRIC_NAMES.items() if key is None))
    if isinstance(metrics, (str, bytes)) or not isinstance(metrics, (list, tuple)):
        raise ValueError("model metrics must be a list of metric names, got %r (%s)" % (metrics, supported))
    act = resolve_activation(activation)
    out, seen = [], set()
    for m in metrics:
        if not isinstance(m, str) or m.lower() not in _METRIC_NAMES:
            raise ValueError("metric %r is not supported by the HIP train step (%s)" % (m, supported))
        kind, key = _METRIC_NAMES[m.lower()]
        if kind in seen:
            raise ValueError("metric %r names a metric already in the list %r" % (m, list(metrics)))
        if kind == "auc" and act != "sigmoid":
            raise ValueError("metric %r needs predictions in [0, 1]: the sigmoid output activation (got %r)"
                             % (m, activation))
        seen.add(kind)
        out.append((key or m, kind))
    return out


RANK_METRIC_FORMS = "hit_rate@K and ndcg@K for an integer K >= 1, mrr (any case)"


def split_rank_metrics(names):
    """The ranking names of a metric list apart from the pointwise ones: returns (pointwise names in their order, to
    hand to ``resolve_metrics``; ranking specs [(key, kind, k)] in their order) with key ``hit_rate@K`` / ``ndcg@K``
    / ``mrr`` (lower case, K as a plain integer: the History column is ``val_`` + key), kind ``hit_rate`` / ``ndcg`` /
    ``mrr`` and k an int or None.  ValueError, listing the accepted forms, for a ranking name without a K (``hit_rate``),
    with a K that is no integer >= 1 (``hit_rate@0``, ``ndcg@x``), ``mrr`` with a K, or a ranking name given twice.
    Anything that is not a list or tuple of names is returned as it is, for ``resolve_metrics`` to refuse."""
    if isinstance(names, (str, bytes)) or not isinstance(names, (list, tuple)):
        return names, []
    point, specs, seen = [], [], set()
    for m in names:
        low = m.lower() if isinstance(m, str) else ""
        kind, at, tail = low.partition("@")
        if kind not in ("hit_rate", "ndcg", "mrr"):
            point.append(m)
            continue
        bad = ValueError("ranking metric %r is not understood (accepted: %s)" % (m, RANK_METRIC_FORMS))
        if kind == "mrr":
            if at:
                raise bad
            key, k = "mrr", None
        else:
            if not (tail.isascii() and tail.isdigit()) or int(tail) < 1:
                raise bad
            k = int(tail)
            key = "%s@%d" % (kind, k)
        if key in seen:
            raise ValueError("ranking metric %r names a column already in the list %r (accepted: %s)"
                             % (m, list(names), RANK_METRIC_FORMS))
        seen.add(key)
        specs.append((key, kind, k))
    return point, specs


def metric_mask(resolved):
    """ANIREC_METRIC_* bits of a resolved metric set (0: nothing beyond the squared error every step keeps)."""
    mask = 0
    for _, kind in resolved:
        mask |= METRIC_BITS[kind]
    return mask


def auc_from_bins(pos, neg):
    """Keras 2.12 AUC() (ROC, 'interpolation' = trapezoidal sum) of the bucketed label masses, in fp64: TP / FP at
    threshold i are the masses of buckets >= i (reverse cumulative sums), TPR = TP / P, FPR = FP / N (0 when P or N is
    0: divide_no_nan)."""
    pos = np.asarray(pos, np.float64)
    neg = np.asarray(neg, np.float64)
    tp = np.cumsum(pos[::-1])[::-1]
    fp = np.cumsum(neg[::-1])[::-1]
    P, N = tp[0], fp[0]
    tpr = tp / P if P > 0 else np.zeros_like(tp)
    fpr = fp / N if N > 0 else np.zeros_like(fp)
    return float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0))


def metric_values(mask, sums, auc_pos, auc_neg, n, se_sum):
    """{kind: epoch value} of the accumulated sums: the sample-weighted means over n ratings, MSE and RMSE from the
    squared-error sum, AUC from the bins."""
    n = max(float(n), 1.0)
    out = {"mse": float(se_sum) / n, "rmse": float(np.sqrt(float(se_sum) / n))}
    for k, kind in enumerate(METRIC_SUM_KINDS):
        if mask & METRIC_BITS[kind]:
            out[kind] = float(sums[k]) / n
    if mask & METRIC_BITS["auc"]:
        out["auc"] = auc_from_bins(auc_pos, auc_neg)
    return out
