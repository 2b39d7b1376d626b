"""anirec_kmeans_fit at the two tables of the full data set (arguments: reps, iterations): the anime table, 17 560 x 128
with K = 64, and a user table of 350 000 x 128 with K = 256, 20 Lloyd iterations each from K rows of the table, beside
the torch route to the same clustering on the same device: ``What @ C.T`` and ``argmax`` (the assign leg), ``index_add_``
of the rows into a zeroed [K, D] table and ``normalize`` (the update leg).  The rows are unit Gaussian directions (no
structure: neither route stops early; ``iterations_run`` says so).

The fit is ONE call that enqueues every iteration, so its legs are not separate calls: ``fit_ms`` is the whole call
(iterations assign passes and updates, the final assign pass and the cluster sizes), ``assign_ms`` one
anirec_kmeans_assign call on the same centroids — the kernel the fit launches, without the moved-rows count — and
``update_ms`` = (fit_ms - (iterations + 1) * assign_ms) / iterations: what is left per iteration for the sums kernel, the
centroid kernel and the launch boundaries.  The torch legs are device events around each leg, summed over the
iterations and divided by them.  Host clock around a device synchronise for the fit, after a warm-up of each route; the
routes alternate inside every repetition and the medians are reported.  Prints one JSON line."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import _lib, ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dim = 128


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def torch_fit(Wh, C0):
    """(C, assign, assign leg ms, update leg ms) of ``iters`` iterations"""
    C = C0.clone()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for j in range(iters):
        ev[j][0].record()
        a = (Wh @ C.T).argmax(dim=1)
        ev[j][1].record()
        S = torch.zeros_like(C).index_add_(0, a, Wh)
        C = torch.nn.functional.normalize(S, dim=1)
        ev[j][2].record()
    torch.cuda.synchronize()
    return C, a, sum(e[0].elapsed_time(e[1]) for e in ev) / iters, sum(e[1].elapsed_time(e[2]) for e in ev) / iters


def shape(name, n, k):
    lib = _lib.load()
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    Wh = ops.rownorm(torch.randn(n, dim, generator=g, device="cuda"))
    C0 = Wh[torch.randperm(n, generator=g, device="cuda")[:k]].contiguous()
    C = C0.clone()
    assign = torch.empty(n, dtype=torch.int32, device="cuda")
    sim = torch.empty(n, device="cuda")
    count = torch.empty(k, dtype=torch.int32, device="cuda")
    info = torch.empty(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.anirec_kmeans_workspace_bytes(n, k, dim)), dtype=torch.uint8, device="cuda")

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fit():
        C.copy_(C0)
        _lib.check(lib.anirec_kmeans_fit(_lib.ptr(Wh), dim, n, _lib.ptr(C), k, iters, _lib.ptr(assign), _lib.ptr(sim),
                                         _lib.ptr(count), _lib.ptr(info), _lib.ptr(ws), ws.numel(), stream()),
                   "anirec_kmeans_fit")

    def assign_only():
        _lib.check(lib.anirec_kmeans_assign(_lib.ptr(Wh), dim, n, _lib.ptr(C0), k, _lib.ptr(assign), _lib.ptr(sim), stream()),
                   "anirec_kmeans_assign")

    for fn in (fit, assign_only, lambda: torch_fit(Wh, C0)):
        timed(fn)                                   # warm-up
    fit_ms, assign_ms, t_assign, t_update, t_whole = [], [], [], [], []
    for _ in range(reps):
        assign_ms.append(timed(assign_only)[0])
        fit_ms.append(timed(fit)[0])
        ms, (_, _, ta, tu) = timed(lambda: torch_fit(Wh, C0))
        t_whole.append(ms)
        t_assign.append(ta)
        t_update.append(tu)
    fit()
    torch.cuda.synchronize()
    tC, ta, _, _ = torch_fit(Wh, C0)
    f, a1 = median(fit_ms), median(assign_ms)
    upd = (f - (iters + 1) * a1) / iters
    return {"table": name, "n_rows": n, "k": k, "iterations": iters, "iterations_run": int(info[0]), "converged": int(info[1]),
            "fit_ms": f, "assign_ms": a1, "update_ms": upd, "assign_gfma_per_s": n * k * dim / a1 / 1e6,
            "torch_fit_ms": median(t_whole), "torch_assign_ms": median(t_assign), "torch_update_ms": median(t_update),
            "torch_over_fit": median(t_whole) / f, "torch_assign_over_assign": median(t_assign) / a1,
            "torch_update_over_update": median(t_update) / upd,
            "dominant_leg": "assign" if a1 > upd else "update",
            # the two routes round differently (fp32 sums in arrival order against exact integer sums), so after 20
            # iterations they agree on most rows, not on all
            "same_cluster_as_torch": float((assign.long() == ta).float().mean())}


out = {"device": torch.cuda.get_device_name(0), "dim": dim, "reps": reps,
       "shapes": [shape("anime", 17_560, 64), shape("user", 350_000, 256)]}
print(json.dumps(out))
