"""anirec_explain_lists and recs.explain_topk at model_recs' batched shape: 100 000 lists of k = 10 rows of a 17 560-row
table, D = 128, m = 3 (arguments: reps, lists, rows), once with histories of 300 entries each and once with a long-tailed
length distribution of the same mean (lognormal, 5 .. 10 000 entries), beside the torch route to the same picks on the
same device: gather the history rows ``Wh[hist]`` ([lists, length, D], lists sorted by length and cut into chunks of at
most 1 GiB, each padded to its own longest history), ``bmm`` with the listed rows, weight, ``torch.topk``.  There is no
earlier kernel to compare against, so the torch route stands in for one.  Host clock around a device synchronise, after a
warm-up call of each route; the routes alternate inside every repetition and the medians are reported.  ``kernel`` is
the entry point alone on preallocated outputs, ``explain_topk`` the whole wrapper (allocation, the error-word read-back
and the hist_row gather included).  The kernel's work per list: n rows of 4 D bytes gathered once, k n chains of D fmas —
the figures reported are the gathered bytes per second and the chain fma rate.  Prints one JSON line."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anime_recommendations_amd import _lib, ops, recs  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n_l = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
n_a = int(sys.argv[3]) if len(sys.argv) > 3 else 17_560
dim, k, m = 128, 10, 3


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


def torch_explain(Wh, idx, off, hist, w, order):
    """(pos, contrib) by gather + bmm + topk; ``order``: the lists by descending history length (computed once, outside
    the timed call, as a user of this route would)"""
    n = idx.shape[0]
    lens = (off[1:] - off[:-1])
    pos = torch.full((n, k, m), -1, dtype=torch.int64, device=idx.device)
    contrib = torch.full((n, k, m), float("nan"), dtype=torch.float32, device=idx.device)
    l0 = 0
    while l0 < n:
        longest = int(lens[order[l0]])
        if longest == 0:
            break
        chunk = max(1, (1 << 30) // (longest * dim * 4))
        ls = order[l0:l0 + chunk]
        at = off[ls].view(-1, 1) + torch.arange(longest, device=idx.device).view(1, -1)
        valid = at < off[ls + 1].view(-1, 1)
        at = torch.where(valid, at, torch.zeros((), dtype=at.dtype, device=at.device))
        H = Wh[hist[at].long()]                                             # [chunk, longest, D]
        G = torch.bmm(Wh[idx[ls].long()], H.transpose(1, 2))               # [chunk, k, longest]
        C = G * w[at].view(len(ls), 1, longest)
        C = torch.where(valid.view(len(ls), 1, longest), C, torch.full((), -float("inf"), device=C.device))
        top, where = torch.topk(C, min(m, longest), dim=2)
        pad = top == -float("inf")                                          # (the weights here are finite: only padding)
        pos[ls, :, :top.shape[2]] = torch.where(pad, torch.full((), -1, device=where.device), where)
        contrib[ls, :, :top.shape[2]] = torch.where(pad, torch.full((), float("nan"), device=top.device), top)
        l0 += chunk
    return pos, contrib


def shape(name, lens):
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    Wh = ops.rownorm(torch.randn(n_a, dim, generator=g, device="cuda"))
    idx = torch.randint(0, n_a, (n_l, k), generator=g, device="cuda", dtype=torch.int32)
    off_h = np.zeros(n_l + 1, np.int64)
    np.cumsum(lens, out=off_h[1:])
    total = int(off_h[-1])
    off = torch.from_numpy(off_h).cuda()
    hist = torch.randint(0, n_a, (total,), generator=g, device="cuda", dtype=torch.int32)
    w = (torch.randint(1, 11, (total,), generator=g, device="cuda").float() / 10.0)
    order = torch.from_numpy(np.argsort(-lens, kind="stable")).cuda()
    lib = _lib.load()
    outs = (torch.empty(n_l, k, m, dtype=torch.int32, device="cuda"), torch.empty(n_l, k, m, device="cuda"),
            torch.empty(n_l, k, m, device="cuda"))
    err = torch.empty(1, dtype=torch.int32, device="cuda")

    def kernel():
        _lib.check(lib.anirec_explain_lists(_lib.ptr(Wh), dim, n_a, _lib.ptr(idx), n_l, k, _lib.ptr(off), _lib.ptr(hist),
                                            _lib.ptr(w), m, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]),
                                            _lib.ptr(err), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "anirec_explain_lists")

    kernel_ms, whole_ms, torch_ms = median_ms([kernel, lambda: recs.explain_topk(Wh, idx, off_h, hist, w, m=m),
                                               lambda: torch_explain(Wh, idx, off, hist, w, order)])
    kernel()
    tp, tc = torch_explain(Wh, idx, off, hist, w, order)
    torch.cuda.synchronize()
    both = (outs[0] >= 0) & (tp >= 0)
    return {"histories": name, "entries": total, "longest": int(lens.max()), "kernel_ms": kernel_ms,
            "explain_topk_ms": whole_ms, "torch_route_ms": torch_ms, "torch_over_kernel": torch_ms / kernel_ms,
            "torch_over_explain_topk": torch_ms / whole_ms,
            "gathered_gb_per_s": total * dim * 4 / kernel_ms / 1e6, "chain_gfma_per_s": total * k * dim / kernel_ms / 1e6,
            "err": int(err.item()), "max_abs_diff_contrib": float((outs[2] - tc)[both].abs().max()),
            "top_pick_agreement": float((outs[0][:, :, 0] == tp[:, :, 0]).float().mean())}


rng = np.random.default_rng(3)
tail = np.clip(rng.lognormal(np.log(200.0), 0.9, n_l), 5, 10_000).astype(np.int64)
out = {"device": torch.cuda.get_device_name(0), "n_lists": n_l, "n_rows": n_a, "dim": dim, "k": k, "m": m, "reps": reps,
       "shapes": [shape("300 each", np.full(n_l, 300, np.int64)), shape("long-tailed", tail)]}
print(json.dumps(out))
