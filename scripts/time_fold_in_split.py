"""ops.fold_in_split against ops.fold_in at the new-anime shape: 48 new rows against a 350 000 x 128 user table, list
lengths from 500 to 200 000 (46 lists spaced geometrically from 500 to 4 000, one of 20 000 and one of 200 000: mean
about 6 200), 100 Adam steps (arguments: reps, steps).  Host clock around a device synchronise, after a warm-up call
of each; whole calls (the normalisation pre-pass, the CSR and chunk-map upload and the error-word read-back included),
the two paths alternately on the same CSR.  Prints one JSON line: both medians, every time, the largest distance
between the two paths' rows and the number of kernel launches of the split call (2 steps + 4)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anime_recommendations_amd import ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
n_table, dim = 350_000, 128
lens = np.concatenate([np.round(500 * 8 ** (np.arange(46) / 45)), [20_000, 200_000]]).astype(np.int64)
g = torch.Generator(device="cuda")
g.manual_seed(7)
T = torch.randn(n_table, dim, generator=g, device="cuda") * 0.05
head = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
nnz = int(offsets[-1])
idx = torch.randint(0, n_table, (nnz,), generator=g, device="cuda", dtype=torch.int32)
rating = torch.randint(0, 11, (nnz,), generator=g, device="cuda").to(torch.float32) / 10
init = torch.randn(dim, generator=g, device="cuda") * 0.05


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(T, head, offsets, idx, rating, init, lr=0.01, steps=steps)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


_, (rows_s, loss_s) = timed(ops.fold_in_split)      # warm-up
_, (rows_w, loss_w) = timed(ops.fold_in)
t_split, t_whole = [], []
for _ in range(reps):
    t_split.append(timed(ops.fold_in_split)[0])
    t_whole.append(timed(ops.fold_in)[0])
med = lambda t: sorted(t)[len(t) // 2]
print(json.dumps({
    "device": torch.cuda.get_device_name(0), "n_new": len(lens), "n_table": n_table, "dim": dim, "steps": steps,
    "ratings": nnz, "mean_list": float(lens.mean()), "longest_list": int(lens.max()),
    "chunks": int(ops.fold_chunk_map(offsets)[0][-1]), "reps": reps,
    "fold_in_split_ms": med(t_split) * 1e3, "fold_in_split_ms_all": [round(x * 1e3, 3) for x in t_split],
    "fold_in_ms": med(t_whole) * 1e3, "fold_in_ms_all": [round(x * 1e3, 3) for x in t_whole],
    "largest_row_distance": float((rows_s - rows_w).abs().max()), "largest_loss_distance": float((loss_s - loss_w).abs().max()),
    "split_launches": 2 * steps + 4, "finite": bool(torch.isfinite(rows_s).all())}))
