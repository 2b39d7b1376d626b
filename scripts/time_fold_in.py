"""ops.fold_in at the serving shape: 100 000 new users x 300 ratings each x 100 Adam steps against a 17 560-anime
table, D = 128 (arguments: reps, users, ratings per user, steps).  Host clock around a device synchronise, after a
warm-up call; whole calls (the normalisation pre-pass, the CSR upload and the error-word read-back included).
Prints one JSON line.  The work is 101 passes (100 steps and the final loss) over every rating: per rating one
gathered 512-byte row, a dot product and an axpy of width D — 4 D flops — so the figures reported are the gathered
bytes per second (the rows come from L2 / Infinity Cache: the normalised table is 9 MB) and the fp32 flop rate."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anime_recommendations_amd import ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n_new = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
per_user = int(sys.argv[3]) if len(sys.argv) > 3 else 300
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 100
n_a, dim = 17_560, 128
g = torch.Generator(device="cuda")
g.manual_seed(7)
A = torch.randn(n_a, dim, generator=g, device="cuda") * 0.05
head = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
offsets = np.arange(n_new + 1, dtype=np.int64) * per_user
idx = torch.randint(0, n_a, (n_new * per_user,), generator=g, device="cuda", dtype=torch.int32)
rating = torch.randint(0, 11, (n_new * per_user,), generator=g, device="cuda").to(torch.float32) / 10
init = torch.randn(dim, generator=g, device="cuda") * 0.05


def call():
    return ops.fold_in(A, head, offsets, idx, rating, init, lr=0.01, steps=steps)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


_, (rows, loss) = timed(call)                       # warm-up
loss0 = ops.fold_in(A, head, offsets[:1025], idx[:1024 * per_user], rating[:1024 * per_user], init, steps=0)[1]
t = [timed(call)[0] for _ in range(reps)]
med = sorted(t)[len(t) // 2]
passes = steps + 1
print(json.dumps({
    "device": torch.cuda.get_device_name(0), "n_new": n_new, "ratings_per_user": per_user, "steps": steps, "dim": dim,
    "n_anime": n_a, "reps": reps, "fold_in_ms": med * 1e3, "fold_in_ms_all": [round(x * 1e3, 3) for x in t],
    "users_per_second": n_new / med, "gathered_tb_per_s": n_new * per_user * passes * dim * 4 / med / 1e12,
    "tflops": 4.0 * dim * n_new * per_user * passes / med / 1e12,
    "mean_loss_start_1024": float(loss0.mean()), "mean_loss_folded_1024": float(loss[:1024].mean()),
    "finite": bool(torch.isfinite(rows).all())}))
