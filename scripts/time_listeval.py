"""ops.list_similarity and recs.list_quality at the evaluation shape: 100 000 lists of k = 10 and of k = 100 rows of a
17 560-row table, D = 128 (arguments: reps, lists, rows), beside the torch route to the same sums on the same device:
gather ``Wh[idx]`` ([n_lists, k, D], in chunks of at most 1 GiB), ``bmm`` with its transpose, strict lower triangle,
row sum and row max.  There is no earlier kernel to compare against, so the torch route stands in for one.  Host clock
around a device synchronise, after a warm-up call of each route; the two routes alternate inside every repetition and the
medians are reported; whole wrapper calls (allocation of the outputs and the error-word read-back included).
``list_quality`` is timed whole, with targets and rating counts, once over the kernel and once with the torch route's
similarities handed to ``recs.list_figures``.  The kernel's work per list: k rows of 4 D bytes gathered once, then
k (k - 1) / 2 chains of D fmas — the figures reported are the gathered bytes per second and the chain fma rate.
Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops, recs  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n_l = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
n_a = int(sys.argv[3]) if len(sys.argv) > 3 else 17_560
dim = 128


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def median_ms(fns):
    """the median ms of each of ``fns``, the routes alternating inside every repetition"""
    for fn in fns:
        timed(fn)                                   # warm-up
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn)[0])
    return [sorted(x)[len(x) // 2] * 1e3 for x in t]


def torch_similarity(Wh, idx):
    """(sim_max, sim_sum) by gather + bmm: every list present, the sums in bmm's order rather than the kernel's"""
    n, k = idx.shape
    sim_max = torch.empty(n, k, dtype=torch.float32, device=idx.device)
    sim_sum = torch.empty(n, k, dtype=torch.float32, device=idx.device)
    chunk = max(1, (1 << 30) // (k * Wh.shape[1] * 4))
    below = torch.ones(k, k, dtype=torch.bool, device=idx.device).tril(-1)
    for l0 in range(0, n, chunk):
        rows = Wh[idx[l0:l0 + chunk].long()]
        G = torch.bmm(rows, rows.transpose(1, 2))
        sim_sum[l0:l0 + chunk] = torch.where(below, G, torch.zeros((), device=G.device)).sum(dim=2)
        mx = torch.where(below, G, torch.full((), -float("inf"), device=G.device)).amax(dim=2)
        mx[:, 0] = 0
        sim_max[l0:l0 + chunk] = mx
    return sim_max, sim_sum


def shape(k):
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    Wh = ops.rownorm(torch.randn(n_a, dim, generator=g, device="cuda"))
    idx = torch.randint(0, n_a, (n_l, k), generator=g, device="cuda", dtype=torch.int32)
    row = torch.arange(n_l, device="cuda")
    anime = torch.where(row % 2 == 0, idx[:, k // 2].long(), torch.zeros_like(row))     # every other target is listed
    count = torch.randint(0, 5000, (n_a,), generator=g, device="cuda").float()
    kernel_ms, torch_ms = median_ms([lambda: ops.list_similarity(Wh, idx), lambda: torch_similarity(Wh, idx)])

    def quality_torch():
        mx, sm = torch_similarity(Wh, idx)
        return recs.list_figures(idx, n_a, mx, sm, row, anime, item_count=count, n_raters=300_000)
    q_kernel_ms, q_torch_ms = median_ms([lambda: recs.list_quality(Wh, idx, k, row, anime, item_count=count,
                                                                    n_raters=300_000), quality_torch])
    (km, ks), (tm, ts) = ops.list_similarity(Wh, idx), torch_similarity(Wh, idx)
    pairs = k * (k - 1) // 2
    return {"k": k, "list_similarity_ms": kernel_ms, "torch_route_ms": torch_ms, "torch_over_kernel": torch_ms / kernel_ms,
            "list_quality_ms": q_kernel_ms, "list_quality_torch_route_ms": q_torch_ms,
            "gathered_gb_per_s": n_l * k * dim * 4 / kernel_ms / 1e6, "chain_gfma_per_s": n_l * pairs * dim / kernel_ms / 1e6,
            "max_abs_diff_sum": float((ks - ts).abs().max()), "max_abs_diff_max": float((km - tm).abs().max()),
            "figures": recs.list_quality(Wh, idx, k, row, anime, item_count=count, n_raters=300_000)}


out = {"device": torch.cuda.get_device_name(0), "n_lists": n_l, "n_rows": n_a, "dim": dim, "reps": reps,
       "shapes": [shape(10), shape(100)]}
print(json.dumps(out))
