"""recs.diverse_topk at the serving shape: 100 000 users x 18 000 anime, pool 100, k 10, D = 128, diversity 0.3
(arguments: reps, users, anime), and the same at D = 32 and 256 with the largest pool anirec_mmr_rerank admits there
(1024 and 128).  Host clock around a device synchronise, after a warm-up call; whole wrapper calls (allocation of the
outputs and the error-word read-back included).  Per shape: ms of ``ops.mmr_rerank`` alone on the pool lists, ms of
the ``ops.predict_topk(pool)`` that produces them, ms of the whole ``recs.diverse_topk`` (the two plus the row
normalisation).  The re-rank's work per list: pool rows of 4 D bytes gathered once, then k - 1 picks of pool chains
of D fmas — the figures reported are the gathered bytes per second and the chain fma rate.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import _lib, ops, recs  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n_u = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
n_a = int(sys.argv[3]) if len(sys.argv) > 3 else 18_000
k, diversity = 10, 0.3
head = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def median_ms(fn):
    timed(fn)                                       # warm-up
    t = sorted(timed(fn)[0] for _ in range(reps))
    return t[len(t) // 2] * 1e3


def shape(dim, pool):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    U = torch.randn(n_u, dim, generator=g, device="cuda") * 0.05
    A = torch.randn(n_a, dim, generator=g, device="cuda") * 0.05
    users = torch.arange(n_u, dtype=torch.int32, device="cuda")
    Wh = ops.rownorm(A)
    cand, p = ops.predict_topk(U, A, head, users, pool)
    mmr = median_ms(lambda: ops.mmr_rerank(Wh, cand, p, k, 1.0 - diversity))
    topk = median_ms(lambda: ops.predict_topk(U, A, head, users, pool))
    whole = median_ms(lambda: recs.diverse_topk(U, A, head, users, k, pool, diversity))
    idx, _, pen = recs.diverse_topk(U, A, head, users, k, pool, diversity)
    return {"dim": dim, "pool": pool, "mmr_rerank_ms": mmr, "predict_topk_pool_ms": topk, "diverse_topk_ms": whole,
            "gathered_gb_per_s": n_u * pool * dim * 4 / mmr / 1e6,
            "chain_gfma_per_s": n_u * (k - 1) * pool * dim / mmr / 1e6,
            "lists_complete": bool((idx >= 0).all()), "mean_pen": float(pen[:, 1:].mean())}


out = {"device": torch.cuda.get_device_name(0), "n_users": n_u, "n_anime": n_a, "k": k, "diversity": diversity, "reps": reps,
       "shapes": [shape(128, 100), shape(32, _lib.mmr_max_cand(32)), shape(256, _lib.mmr_max_cand(256))]}
print(json.dumps(out))
