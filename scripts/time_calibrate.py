"""ops.calibrate_rerank and ops.list_calibration at the serving shape: 100 000 lists, pool 100, k 10, 43 categories,
calibration 0.5 (arguments: reps, lists, pool, n_cat), beside a torch route to the same picks on the same GPU: k
rounds of batched int64 tensors, each round the [n_lists, pool, n_cat] terms |p_c Q' - q'_c P| of every candidate,
their sum, the fp64 quotient, the fp32 value and an argmax.  Host clock around a device synchronise, after a warm-up
call; whole wrapper calls (allocation of the outputs and the error-word read-back included); the two kernel calls are
timed ``inner`` calls at a time so that a sample is not a fraction of a millisecond.  The torch route must return the
kernel's picks and pen bits (``same_picks``), or its time means nothing.  The category table has 18 000 rows of density
3 / n_cat + 0.02; candidates are random rows, scores descending uniforms, profile counts below 50.  Prints one JSON
line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anime_recommendations_amd import ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n_lists = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
pool = int(sys.argv[3]) if len(sys.argv) > 3 else 100
n_cat = int(sys.argv[4]) if len(sys.argv) > 4 else 43
n_rows, k, cal, inner = 18_000, 10, 0.5, 10


def timed(fn, n=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, out


def median_ms(fn, n=1):
    timed(fn)                                       # warm-up
    t = sorted(timed(fn, n)[0] for _ in range(reps))
    return t[len(t) // 2] * 1e3, (t[-1] - t[0]) * 1e3


g = torch.Generator(device="cuda")
g.manual_seed(11)
dense = torch.rand(n_rows, n_cat, generator=g, device="cuda") < min(0.5, 3 / n_cat + 0.02)
cw = (n_cat + 31) // 32
shifts = torch.arange(n_cat, device="cuda")
words = torch.zeros(n_rows, cw, dtype=torch.int64, device="cuda")
words.scatter_add_(1, (shifts >> 5)[None, :].expand(n_rows, n_cat), dense.long() << (shifts & 31)[None, :])
cat_bits = torch.from_numpy(words.cpu().numpy().astype(np.uint32).view(np.int32)).cuda()
cand = torch.randint(0, n_rows, (n_lists, pool), generator=g, device="cuda", dtype=torch.int32)
score = torch.rand(n_lists, pool, generator=g, device="cuda").sort(dim=1, descending=True).values
profile = torch.randint(0, 50, (n_lists, n_cat), generator=g, device="cuda", dtype=torch.int32)
B = dense.long()


def torch_route():
    """the definition, k rounds over [n_lists, pool, n_cat] int64 tensors: (idx, pen) of the picks"""
    c32 = torch.tensor(cal, dtype=torch.float32, device="cuda")
    omc = torch.tensor(1.0, device="cuda") - c32
    Bc = B[cand.long()]
    pop = Bc.sum(dim=2)
    p = profile.long()
    P = p.sum(dim=1)
    q = torch.zeros_like(p)
    Q = torch.zeros_like(P)
    live = torch.ones(n_lists, pool, dtype=torch.bool, device="cuda")
    ls = omc * score
    rows = torch.arange(n_lists, device="cuda")
    out_idx = torch.empty(n_lists, k, dtype=torch.int32, device="cuda")
    out_pen = torch.empty(n_lists, k, dtype=torch.float32, device="cuda")
    for s in range(k):
        Qp = Q[:, None] + pop
        num = (p[:, None, :] * Qp[:, :, None] - (q[:, None, :] + Bc) * P[:, None, None]).abs_().sum(dim=2)
        den = 2 * P[:, None] * Qp
        pen = (num.double() / den.clamp(min=1).double()).float()
        pen = torch.where(Qp == 0, torch.ones_like(pen), pen)
        pen = torch.where(P[:, None] == 0, torch.zeros_like(pen), pen)
        val = torch.where(live, ls - c32 * pen, torch.full_like(ls, float("-inf")))
        best = val.argmax(dim=1)                    # the first of equal maxima: the lowest position
        out_idx[:, s] = cand[rows, best]
        out_pen[:, s] = pen[rows, best]
        live[rows, best] = False
        q += Bc[rows, best]
        Q += pop[rows, best]
    return out_idx, out_pen


rerank_ms, rerank_spread = median_ms(lambda: ops.calibrate_rerank(cat_bits, n_cat, cand, score, profile, k, cal), inner)
idx, pos, _, pen = ops.calibrate_rerank(cat_bits, n_cat, cand, score, profile, k, cal)
listcal_ms, listcal_spread = median_ms(lambda: ops.list_calibration(cat_bits, n_cat, idx, profile), inner)
torch_ms, torch_spread = median_ms(torch_route)
t_idx, t_pen = torch_route()
plain = ops.list_calibration(cat_bits, n_cat, cand[:, :k].contiguous(), profile)[0]
out = {"device": torch.cuda.get_device_name(0), "n_lists": n_lists, "pool": pool, "k": k, "n_cat": n_cat,
       "calibration": cal, "reps": reps, "inner": inner,
       "calibrate_rerank_ms": rerank_ms, "calibrate_rerank_spread_ms": rerank_spread,
       "list_calibration_ms": listcal_ms, "list_calibration_spread_ms": listcal_spread,
       "torch_route_ms": torch_ms, "torch_route_spread_ms": torch_spread,
       "torch_over_kernel": torch_ms / rerank_ms,
       "same_picks": bool(torch.equal(idx, t_idx) and torch.equal(pen.view(torch.int32), t_pen.view(torch.int32))),
       "list_calibration_is_out_pen": bool(torch.equal(
           ops.list_calibration(cat_bits, n_cat, idx, profile)[0].view(torch.int32), pen[:, -1].contiguous().view(torch.int32))),
       "mean_miscalibration": float(pen[:, -1].mean()), "mean_miscalibration_topk": float(plain.mean()),
       "mean_score": float(score.gather(1, pos.long()).mean()),
       "mean_score_topk": float(score[:, :k].mean())}
print(json.dumps(out))
