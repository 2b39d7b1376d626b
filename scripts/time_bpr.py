"""The BPR kernels at the full data set's shape (arguments: reps): one epoch (ceil(pairs / 131072) steps of 131072
triples) and a whole default fit (30 epochs) of ``ops.bpr_steps`` over 350 000 users x 300 liked of 17 560 items with the
long-tailed law of time_als.py, at widths 64 and 128 with BPR_DEFAULTS — beside a torch route on the same device that
takes the SAME triples (``ops.bpr_sample``'s, drawn and cleared of dropped slots before the clock starts, so the timed
loop reads nothing back) through gather, ``torch.sigmoid`` and ``index_add_``: the usual sparse SGD step, fp32 float
atomics, not reproducible from run to run.  The torch route is timed for one epoch; its whole fit is that times 30, said
so in the line.  Host clock around a device synchronise, after a
warm-up of each route; the routes alternate inside every repetition and the medians are reported.  Prints one JSON line
and saves it as profiles/time_bpr.json.  With ``--profile`` instead: 100 steps at each width and nothing else, the run
``rocprofv3 --kernel-trace --stats`` takes the per-kernel times from (profiles/bpr_kernel_stats.csv)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from anime_recommendations_amd import components as C, ops  # noqa: E402

PROFILE = "--profile" in sys.argv
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not PROFILE else 3
N_USERS, N_ITEMS, PER_USER = 350_000, 17_560, 300
PAR = C.BPR_DEFAULTS
BATCH, TRIES, LR, REG, EPOCHS, SEED = PAR["batch"], PAR["tries"], PAR["lr"], PAR["reg"], PAR["epochs"], PAR["seed"]
SAMPLE_STEPS = 64            # steps of triples one ops.bpr_sample call draws (100 MB); the whole epoch's stay resident


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def pairs():
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    w = (torch.arange(N_ITEMS, device="cuda", dtype=torch.float64) + 50.0) ** -0.8
    cdf = torch.cumsum(w / w.sum(), 0)
    u = torch.rand(N_USERS * PER_USER, generator=g, device="cuda", dtype=torch.float64)
    item = torch.searchsorted(cdf, u).clamp(max=N_ITEMS - 1)
    user = torch.arange(N_USERS, device="cuda").repeat_interleave(PER_USER)
    key = torch.unique(user * N_ITEMS + item)                   # the distinct pairs, rows and items ascending
    pu, idx = (key // N_ITEMS).to(torch.int32), (key % N_ITEMS).to(torch.int32)
    off = torch.zeros(N_USERS + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.bincount(pu.long(), minlength=N_USERS), 0)
    return off, idx, pu


def start(F):
    g = torch.Generator(device="cuda")
    g.manual_seed(F)
    X = torch.randn(N_USERS, F, generator=g, device="cuda") * 0.01
    Y = torch.randn(N_ITEMS, F, generator=g, device="cuda") * 0.01
    X[:, -1], Y[:, -1] = 1.0, 0.0
    return X, Y


def kept_triples(trip):
    """per step (u, i, j) int64 of the kept slots: the filtering (a read-back of the count) happens here, untimed"""
    out = []
    for t in range(trip.shape[0]):
        tr = trip[t]
        tr = tr[tr[:, 2] >= 0].long()
        out.append((tr[:, 0].contiguous(), tr[:, 1].contiguous(), tr[:, 2].contiguous()))
    return out


def torch_steps(X, Y, steps):
    """the usual sparse SGD step on given triples: every slot adds lr (its gradient - reg its row) to its three rows"""
    for u, i, j in steps:
        x, yi, yj = X[u], Y[i], Y[j]
        d = yi - yj
        g = torch.sigmoid(-(x * d).sum(1, keepdim=True))
        du = LR * (g * d - REG * x)
        du[:, -1] = 0.0                                          # the bias column of the user rows stays 1
        X.index_add_(0, u, du)
        Y.index_add_(0, i, LR * (g * x - REG * yi))
        Y.index_add_(0, j, LR * (-g * x - REG * yj))


def width(F, off, idx, pu):
    per = -(-int(idx.numel()) // BATCH)
    ws = torch.empty(ops.bpr_workspace_bytes(N_USERS, N_ITEMS, F, BATCH), dtype=torch.uint8, device="cuda")
    X, Y = start(F)

    def epoch(e):
        return ops.bpr_steps(X, Y, off, idx, pu, BATCH, TRIES, SEED, e * per, per, LR, REG, True, workspace=ws, check=False)

    def fit():
        Xf, Yf = start(F)
        flags = [ops.bpr_steps(Xf, Yf, off, idx, pu, BATCH, TRIES, SEED, e * per, per, LR, REG, True, workspace=ws,
                               check=False) for e in range(EPOCHS)]
        return flags

    Xt, Yt = start(F)

    def torch_epoch():
        torch_steps(Xt, Yt, trips)

    ops.bpr_sample(off, idx, pu, N_ITEMS, BATCH, TRIES, SEED, 0, 1, check=False)
    sample_ms, _ = timed(lambda: ops.bpr_sample(off, idx, pu, N_ITEMS, BATCH, TRIES, SEED, 0, SAMPLE_STEPS, check=False))
    trips = []
    for s0 in range(0, per, SAMPLE_STEPS):
        trips += kept_triples(ops.bpr_sample(off, idx, pu, N_ITEMS, BATCH, TRIES, SEED, s0, min(SAMPLE_STEPS, per - s0),
                                             check=False)[0])
    timed(lambda: epoch(0))
    timed(torch_epoch)
    a, b = [], []
    for r in range(reps):
        ms, (counts, err) = timed(lambda: epoch(1 + r))
        a.append(ms)
        b.append(timed(torch_epoch)[0])
    del trips
    kept = float(counts[:, 0].double().mean())
    fit_ms, flags = timed(fit)
    flag = 0
    for _, f in flags:
        flag |= int(f.item())
    step_us = median(a) / per * 1e3
    return {"factors": F, "pairs": int(idx.numel()), "steps_per_epoch": per, "epoch_ms": median(a),
            "torch_epoch_ms": median(b), "torch_over_kernel": median(b) / median(a), "fit_ms": fit_ms,
            "fit_epochs": EPOCHS, "torch_fit_ms_as_30_epochs": 30 * median(b), "step_us": step_us,
            "triples_per_us": kept / step_us, "kept_per_step": kept,
            "dropped_per_step": float(counts[:, 1].double().mean()),
            "atomic_added_GB_per_s": 3 * kept * F * 8 / step_us / 1e3, "workspace_MB": ws.numel() / 1e6,
            "sample_64_steps_ms": sample_ms, "flag": flag}


off, idx, pu = pairs()
if PROFILE:
    for F in (64, 128):
        X, Y = start(F)
        ops.bpr_steps(X, Y, off, idx, pu, BATCH, TRIES, SEED, 0, 100, LR, REG, True, check=False)
    torch.cuda.synchronize()
    sys.exit(0)
line = json.dumps({"device": torch.cuda.get_device_name(0), "reps": reps, "batch": BATCH, "tries": TRIES, "lr": LR,
                   "reg": REG, "widths": [width(64, off, idx, pu), width(128, off, idx, pu)]})
print(line)
with open(os.path.join(ROOT, "profiles", "time_bpr.json"), "w") as f:
    f.write(line + "\n")
