"""NumPy restatement of the Keras 2.12 metrics the GPU accumulates (include/anirec.h, ANIREC_METRIC_*), per rating in
fp32 from the head's y, p and the target t (the forward intermediates the oracle's step and evaluate return), summed
in fp64.  Each kind cites the Keras function it restates."""
import numpy as np

from oracle import anirec_oracle as orc

f32 = np.float32
EPS = f32(1e-7)                      # keras.backend.epsilon()
KINDS = ("mae", "mape", "msle", "logcosh", "bce", "accuracy")   # the order of anirec_metric_acc.sum
BINS = 200                           # keras.metrics.AUC(num_thresholds=200)
ONE = 1 << 20                        # fixed-point label mass of one rating in the AUC bins


def per_rating(kind, y, p, t, act):
    """fp32 per-rating value of one scalar kind"""
    y, p, t = (np.asarray(x, f32) for x in (y, p, t))
    e = (p - t).astype(f32)
    if kind == "mae":            # keras.metrics.mean_absolute_error: mean(abs(y_pred - y_true))
        return np.abs(e)
    if kind == "mape":           # keras.metrics.mean_absolute_percentage_error: 100 * abs((t - p) / max(abs(t), eps))
        return (f32(100) * (np.abs(e) / np.maximum(np.abs(t), EPS))).astype(f32)
    if kind == "msle":           # keras.metrics.mean_squared_logarithmic_error
        d = (np.log(np.maximum(p, EPS) + f32(1), dtype=f32) - np.log(np.maximum(t, EPS) + f32(1), dtype=f32))
        return (d * d).astype(f32)
    if kind == "logcosh":        # keras.metrics.logcosh: x + softplus(-2x) - log(2), x = y_pred - y_true
        return orc.loss_terms("log_cosh", p, t)[0]
    if kind == "bce":            # keras.metrics.binary_crossentropy (from the logits of a sigmoid: _keras_logits)
        if act == "sigmoid":
            return orc.bce_from_logits(y, t, f32)
        return orc.loss_terms("binary_crossentropy", p, t)[0]
    if kind == "accuracy":       # keras.metrics.binary_accuracy: equal(y_true, cast(y_pred > 0.5))
        return (t == (p > f32(0.5)).astype(f32)).astype(f32)
    raise ValueError(kind)


def auc_bins(p, t):
    """keras.utils.metrics_utils.update_confusion_matrix_variables, thresholds_distributed_evenly: bucket
    relu(ceil(p * 199) - 1) (fp32 product); label mass t and 1 - t, here in units of 2^-20 (rint of the clamped t)"""
    p, t = np.asarray(p, f32), np.asarray(t, f32)
    b = np.clip(np.ceil(p * f32(BINS - 1)) - f32(1), 0, BINS - 1).astype(np.int64)
    wt = np.rint(np.clip(t, f32(0), f32(1)) * f32(ONE)).astype(np.uint64)
    pos = np.zeros(BINS, np.uint64)
    neg = np.zeros(BINS, np.uint64)
    np.add.at(pos, b, wt)
    np.add.at(neg, b, np.uint64(ONE) - wt)
    return pos, neg


def auc_from_bins(pos, neg):
    """keras.metrics.AUC.result(), ROC curve, summation_method='interpolation': TP / FP at threshold i are the masses
    of buckets >= i; the trapezoidal sum of TPR over FPR (divide_no_nan)"""
    pos, neg = np.asarray(pos, np.float64), np.asarray(neg, np.float64)
    tp, fp = np.cumsum(pos[::-1])[::-1], np.cumsum(neg[::-1])[::-1]
    tpr = tp / tp[0] if tp[0] > 0 else np.zeros(BINS)
    fpr = fp / fp[0] if fp[0] > 0 else np.zeros(BINS)
    return float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0))


def auc_threshold_loop(p, t):
    """keras.metrics.AUC by its definition: for each of the 200 thresholds [-eps, 1/199, ..., 198/199, 1 + eps] the
    confusion counts of 'p > threshold', then the same trapezoidal sum"""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    thr = [-1e-7] + [i / (BINS - 1) for i in range(1, BINS - 1)] + [1 + 1e-7]
    P, N = t.sum(), (1 - t).sum()
    tpr = np.array([(t * (p > h)).sum() / P for h in thr])
    fpr = np.array([((1 - t) * (p > h)).sum() / N for h in thr])
    return float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0))


class Acc:
    """fp64 sums of every kind + the AUC bins + the count and squared-error sum, over any number of batches"""

    def __init__(self):
        self.sum = {k: 0.0 for k in KINDS}
        self.pos = np.zeros(BINS, np.uint64)
        self.neg = np.zeros(BINS, np.uint64)
        self.n = 0
        self.se = 0.0
        self.near_half = 0       # ratings whose p lies within 1e-5 of the accuracy threshold

    def add(self, y, p, t, act):
        for k in KINDS:
            self.sum[k] += float(np.sum(per_rating(k, y, p, t, act), dtype=np.float64))
        if act == "sigmoid":
            a, b = auc_bins(p, t)
            self.pos += a
            self.neg += b
        self.n += len(t)
        e = (np.asarray(p, f32) - np.asarray(t, f32)).astype(f32)
        self.se += float(np.sum(e * e, dtype=np.float64))
        self.near_half += int(np.sum(np.abs(np.asarray(p, np.float64) - 0.5) < 1e-5))

    def values(self):
        v = {k: s / self.n for k, s in self.sum.items()}
        v["mse"] = self.se / self.n
        v["rmse"] = float(np.sqrt(self.se / self.n))
        v["auc"] = auc_from_bins(self.pos, self.neg)
        return v


def train_steps(state, ui, ai, t, starts, counts, lr, loss, act, acc=None):
    """orc.train_step over the batches, the metrics of each batch's training-mode forward added to ``acc``"""
    acc = acc or Acc()
    for s, c in zip(starts, counts):
        tt = t[s:s + c]
        _, f, _ = orc.train_step(state, ui[s:s + c], ai[s:s + c], tt, lr, loss=loss, activation=act)
        acc.add(f["y"], f["p"], tt, act)
    return acc


def evaluate(state, ui, ai, t, act, loss="binary_crossentropy"):
    """the metrics of a validation pass (BN inference mode)"""
    r = orc.evaluate(state, ui, ai, t, loss=loss, activation=act)
    acc = Acc()
    acc.add(r["y"], r["p"], t, act)
    return acc
