"""EASE at the full data set's size (arguments: reps [--n N_ITEMS] [--users N_USERS]), beside the torch routes on the same
device.

inverse   A = B B^T + 500 I for 17 560 items x 70 000 users (about 100 liked anime a user, item popularity long-tailed):
          ``ops.spd_inverse`` (anirec_spd_inverse; its clone of A included) beside ``torch.linalg.inv`` in fp64 and in
          fp32 and ``torch.linalg.cholesky`` + ``torch.cholesky_inverse`` in fp64; the residual max |A P - I| of each.
fit       the whole ``recs.ease_fit`` (bit rows, the count rows in COOC_BATCH batches, the inverse, the weights).
lists     ``recs.ease_topk(k=10)`` (anirec_ease_scores + the exact select, 4096 users a call) for 10 000 and 100 000
          users x 300 history entries, and ``ops.ease_scores`` alone, beside ``torch.sparse.mm`` of the histories' CSR
          [users, items] against W followed by ``topk``; how often both name the same best item.

hipEvent timing on the current stream after a warm-up of each route; the routes alternate inside every repetition and the
medians are reported, whichever side wins.  Also stated: the operations and bytes each phase needs (the inverse: 2 n^3
fp64 operations and one read and one write of A per block step; the score rows: one W row of 4 n bytes per history
entry, 4 n bytes written per list) against the nominal fp64 matrix rate and HBM rate.
A torch route that cannot get its workspace at the size asked for is reported under ``failed_routes`` and the others go
on; ``--n`` / ``--users`` give a smaller problem to compare at (saved as profiles/time_ease_n<N>.json).
Prints one JSON line and saves it as profiles/time_ease.json."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anime_recommendations_amd import ops, recs  # noqa: E402


def flag(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else 3
N_ITEMS, N_USERS = flag("--n", 17_560), flag("--users", 70_000)
LIKED, HIST, TOP, LIST_BATCH, REG = 100, 300, 10, 4096, 500.0
USERS = (10_000, 100_000)
HBM_TBS, F64_MATRIX_TFLOPS = 8.0, 78.6      # MI355X, nominal: peak HBM3E rate; peak fp64 matrix rate


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def race(routes, reps, failed=None):
    """{name: median ms}: a warm-up of each route, then the routes alternating inside every repetition.  A route whose
    warm-up raises a RuntimeError (a library that cannot get its workspace at this size) is reported in ``failed``
    (name -> message) with None as its time, and the others go on."""
    routes = dict(routes)
    failed = {} if failed is None else failed
    for k, fn in list(routes.items()):
        try:
            timed(fn)
        except RuntimeError as e:
            failed[k] = str(e).splitlines()[0][:200]
            del routes[k]
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ms[k].append(timed(fn)[0])
    return dict({k: None for k in failed}, **{k: median(v) for k, v in ms.items()})


def say(what):
    print("time_ease: " + what, file=sys.stderr, flush=True)


def residual(A, P):
    """max |A P - I| in fp64, a block of rows at a time"""
    worst = 0.0
    for r0 in range(0, A.shape[0], 2048):
        blk = A[r0:r0 + 2048] @ P.double()
        blk.diagonal(r0).sub_(1.0)
        worst = max(worst, float(blk.abs().max()))
    return worst


rng = np.random.default_rng(11)
p = 1.0 / np.arange(1, N_ITEMS + 1) ** 0.8
p /= p.sum()
user = np.repeat(np.arange(N_USERS, dtype=np.int32), LIKED)
item = rng.choice(N_ITEMS, N_USERS * LIKED, p=p).astype(np.int32)
rating = np.ones(len(user), np.float32)
out = {"device": torch.cuda.get_device_name(0), "reps": reps, "n_items": N_ITEMS, "n_users": N_USERS,
       "pairs_drawn": int(len(user)), "reg": REG, "block": int(ops._lib.load().anirec_spd_inverse_block()),
       "nominal_hbm_tb_per_s": HBM_TBS, "nominal_fp64_matrix_tflops": F64_MATRIX_TFLOPS}

# ---- the whole fit, then the matrix it inverts ------------------------------------------------------------------------
say("the fit")
fit_ms = race({"ease_fit_ms": lambda: recs.ease_fit(user, item, rating, N_USERS, N_ITEMS, reg=REG)}, reps)
out.update(fit_ms)
fit = recs.ease_fit(user, item, rating, N_USERS, N_ITEMS, reg=REG)
out["liked_pairs"] = int(fit["pop"].sum())
bits = recs.item_bits(torch.as_tensor(user).cuda(), torch.as_tensor(item).cuda(), N_USERS, N_ITEMS)
A = torch.empty(N_ITEMS, N_ITEMS, dtype=torch.float64, device="cuda")
q = torch.arange(N_ITEMS, dtype=torch.int32, device="cuda")
for q0 in range(0, N_ITEMS, recs.COOC_BATCH):
    A[q0:q0 + recs.COOC_BATCH] = ops.cooc_scores(bits, N_USERS, q[q0:q0 + recs.COOC_BATCH], count=True)[1]
A.diagonal().add_(REG)
A32 = A.float()
del bits

inverse = {"spd_inverse_ms": lambda: ops.spd_inverse(A)[0],
           "torch_inv_fp64_ms": lambda: torch.linalg.inv(A),
           "torch_inv_fp32_ms": lambda: torch.linalg.inv(A32),
           "torch_cholesky_inverse_fp64_ms": lambda: torch.cholesky_inverse(torch.linalg.cholesky(A))}
say("the inverse routes")
torch.cuda.empty_cache()
out["failed_routes"] = {}
inv_ms = race(inverse, reps, out["failed_routes"])
say("the residuals")
out.update(inv_ms)
P, info = ops.spd_inverse(A)
out["info"] = int(info.item())
out["residual_spd_inverse"] = residual(A, P)
del P
for name, fn in list(inverse.items())[1:]:
    out["residual_" + name[:-3]] = None if inv_ms[name] is None else residual(A, fn())
best_torch64 = min([inv_ms[k] for k in ("torch_inv_fp64_ms", "torch_cholesky_inverse_fp64_ms") if inv_ms[k] is not None],
                   default=None)
steps = -(-N_ITEMS // out["block"])
flops, step_bytes = 2.0 * N_ITEMS ** 3, 2.0 * 8 * N_ITEMS ** 2
s = inv_ms["spd_inverse_ms"] / 1e3
out.update({"inverse_winner_fp64": None if best_torch64 is None else
            "libanirec" if inv_ms["spd_inverse_ms"] < best_torch64 else "torch",
            "torch_fp64_over_ours": None if best_torch64 is None else best_torch64 / inv_ms["spd_inverse_ms"],
            "inverse_block_steps": steps, "inverse_fp64_flops": flops, "inverse_tflops": flops / s / 1e12,
            "inverse_bytes_hbm": steps * step_bytes, "inverse_tb_per_s": steps * step_bytes / s / 1e12,
            "inverse_floor_ms_at_matrix_rate": flops / (F64_MATRIX_TFLOPS * 1e12) * 1e3,
            "inverse_floor_ms_at_hbm_rate": steps * step_bytes / (HBM_TBS * 1e12) * 1e3})
del A, A32

# ---- score rows and lists ---------------------------------------------------------------------------------------------
W = fit["W"]


def ours_scores(off, hist):
    for l0 in range(0, len(off) - 1, LIST_BATCH):
        ops.ease_scores(W, off[l0:l0 + LIST_BATCH + 1], hist, None, check=False)


def torch_route(hist, n_lists):
    res = []
    ones = torch.ones(LIST_BATCH * HIST, dtype=torch.float32, device="cuda")
    for l0 in range(0, n_lists, LIST_BATCH):
        n = min(LIST_BATCH, n_lists - l0)
        crow = torch.arange(0, (n + 1) * HIST, HIST, device="cuda", dtype=torch.int64)
        H = torch.sparse_csr_tensor(crow, hist[l0 * HIST:(l0 + n) * HIST].long(), ones[:n * HIST], size=(n, N_ITEMS))
        res.append(torch.topk(torch.sparse.mm(H, W), TOP, dim=1))
    return res


out["users"] = {}
for n_lists in USERS:
    say("lists for %d users" % n_lists)
    hist = torch.as_tensor(rng.choice(N_ITEMS, n_lists * HIST, p=p).astype(np.int32)).cuda()
    off = np.arange(0, (n_lists + 1) * HIST, HIST, dtype=np.int64)
    r = race({"ease_scores_ms": lambda: ours_scores(off, hist),
              "ease_topk_ms": lambda: recs.ease_topk(fit, off, hist, None, TOP, batch=LIST_BATCH),
              "torch_sparse_topk_ms": lambda: torch_route(hist, n_lists)}, reps)
    idx, _ = recs.ease_topk(fit, off, hist, None, TOP, batch=LIST_BATCH)
    ti = torch.cat([t.indices for t in torch_route(hist, n_lists)])
    row_bytes, write_bytes = n_lists * HIST * 4.0 * N_ITEMS, n_lists * 4.0 * N_ITEMS
    s = r["ease_scores_ms"] / 1e3
    r.update({"torch_over_ours_topk": r["torch_sparse_topk_ms"] / r["ease_topk_ms"],
              "winner": "libanirec" if r["ease_topk_ms"] < r["torch_sparse_topk_ms"] else "torch",
              "same_best_item": float((idx[:, 0].long() == ti[:, 0]).float().mean()),
              "terms": float(n_lists) * HIST * N_ITEMS, "terms_per_s": float(n_lists) * HIST * N_ITEMS / s,
              "w_row_read_bytes": row_bytes, "w_row_read_tb_per_s": row_bytes / s / 1e12,
              "score_write_bytes_hbm": write_bytes,
              "floor_ms_reading_w_once_per_slab_and_writing": (4.0 * N_ITEMS * N_ITEMS * -(-n_lists // LIST_BATCH)
                                                               + write_bytes) / (HBM_TBS * 1e12) * 1e3})
    out["users"][str(n_lists)] = r
    del hist

line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
name = "time_ease.json" if N_ITEMS == 17_560 else "time_ease_n%d.json" % N_ITEMS
with open(os.path.join(ROOT, "profiles", name), "w") as f:
    f.write(line + "\n")
