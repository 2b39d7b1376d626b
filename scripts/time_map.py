"""anirec_tsne_forces / anirec_tsne_fit at the two tables of the full data set (arguments: reps, iterations of the anime
fit, iterations of the user fit): 17 560 rows and 350 000 rows, points N(0, 1) * 20 under a random symmetric graph of 90
drawn neighbours a row (about 180 stored pairs a row once symmetrised), beside a torch route to the same iteration on the
same device: pairwise differences in row chunks of at most 2^26 pairs, fp32 float sums, the stored pairs through
``index_add_``, the same gains and momentum.

``forces_ms`` is one anirec_tsne_forces call (all pairs, the stored pairs, no update), ``fit_ms`` one anirec_tsne_fit call
of ``iterations`` iterations — ONE call that enqueues everything — and ``fit_iteration_ms`` its share per iteration.  The
user table's fit runs few iterations by default (an iteration is 1.2e11 pairs): ``fit_1000_ms_projected`` is
1000 * fit_iteration_ms, a projection, not a measurement.  Host clock around a device synchronise, after a warm-up of
each route; the routes alternate inside every repetition and the medians are reported.  Prints one JSON line (and the
warm-up times on stderr as it goes)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops, recs  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters_small = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
iters_big = int(sys.argv[3]) if len(sys.argv) > 3 else 5
NEIGHBOURS, EXAG, CHUNK_PAIRS = 90, 12.0, 1 << 26


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def torch_sums(Y, r, idx, val):
    """(R [n, 2], A [n, 2], Z) in fp32 with float sums"""
    n = Y.shape[0]
    chunk = max(1, CHUNK_PAIRS // n)
    R = torch.empty_like(Y)
    Z = torch.zeros((), device=Y.device)
    for b in range(0, n, chunk):
        d = Y[b:b + chunk, None, :] - Y[None, :, :]
        q = 1.0 / (1.0 + d.square().sum(dim=2))
        Z += q.sum() - d.shape[0]
        R[b:b + chunk] = ((q * q)[:, :, None] * d).sum(dim=1)
    d = Y[r] - Y[idx]
    a = val / (1.0 + d.square().sum(dim=1))
    return R, torch.zeros_like(Y).index_add_(0, r, a[:, None] * d), Z


def torch_fit(Y0, r, idx, val, iters, exag_iters, lr):
    Y = Y0.clone()
    n = Y.shape[0]
    V, G = torch.zeros_like(Y), torch.ones_like(Y)
    for t in range(iters):
        early = t < exag_iters
        R, A, Z = torch_sums(Y, r, idx, val)
        grad = 4.0 * ((EXAG if early else 1.0) * A / (2.0 * n) - R / Z)
        G = torch.where(torch.sign(grad) != torch.sign(V), G + 0.2, G * 0.8).clamp_(min=0.01)
        V = (0.5 if early else 0.8) * V - lr * G * grad
        Y = Y + V
    return Y


def shape(name, n, iters):
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    Y0 = (torch.randn(n, 2, generator=g, device="cuda") * 20).contiguous()
    nbr = torch.randint(0, n - 1, (n, NEIGHBOURS), generator=g, device="cuda")
    nbr = nbr + (nbr >= torch.arange(n, device="cuda")[:, None])            # never the row itself
    p = torch.full((n, NEIGHBOURS), 1.0 / NEIGHBOURS, dtype=torch.float64, device="cuda")
    off, idx, val = recs._map_symmetrise(nbr, p, n)
    r = torch.arange(n, device="cuda").repeat_interleave(off[1:] - off[:-1])
    idx_l = idx.long()
    lr, exag_iters = recs.map_lr(n, EXAG), iters // 4
    routes = {"forces": lambda: ops.tsne_forces(Y0, off, idx, val),
              "fit": lambda: ops.tsne_fit(Y0, off, idx, val, iters, exag_iters, EXAG, lr),
              "torch_forces": lambda: torch_sums(Y0, r, idx_l, val),
              "torch_fit": lambda: torch_fit(Y0, r, idx_l, val, iters, exag_iters, lr)}
    ms = {k: [] for k in routes}
    for k, fn in routes.items():
        print("%s: %s warm-up %.1f ms" % (name, k, timed(fn)[0]), file=sys.stderr, flush=True)
    for _ in range(reps):
        for k, fn in routes.items():                # the routes alternate inside a repetition
            ms[k].append(timed(fn)[0])
    m = {k: median(v) for k, v in ms.items()}
    Yl, Yt = routes["fit"]()[0], routes["torch_fit"]()
    return {"table": name, "n_rows": n, "stored_pairs": int(idx.numel()), "iterations": iters, "learning_rate": lr,
            "forces_ms": m["forces"], "pairs_per_s": n * (n - 1) / m["forces"] * 1e3,
            "fit_ms": m["fit"], "fit_iteration_ms": m["fit"] / iters, "fit_1000_ms_projected": m["fit"] / iters * 1000,
            "torch_forces_ms": m["torch_forces"], "torch_fit_ms": m["torch_fit"],
            "torch_fit_iteration_ms": m["torch_fit"] / iters,
            "torch_over_forces": m["torch_forces"] / m["forces"], "torch_over_fit": m["torch_fit"] / m["fit"],
            "all_ms": ms,
            # the two routes round differently (fp32 float sums against exact integer sums) and the dynamics amplify it
            "largest_coordinate_difference_to_torch": float((Yl - Yt).abs().max())}


out = {"device": torch.cuda.get_device_name(0), "reps": reps,
       "shapes": [shape("anime", 17_560, iters_small), shape("user", 350_000, iters_big)]}
print(json.dumps(out))
