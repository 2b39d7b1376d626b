"""ops.predict_rank against the route to the same ranks that exists without it, at 4 096 targets x 17 560 anime,
D = 128 (a size at which the whole-ranking route still fits): ops.predict_topk(k = n_anime), one query per target
under its user's mask with the target's bit cleared, plus the search for the target in each list.  The two are timed
alternately in one process, host clock around a device synchronise, after a warm-up of each; the ranks are compared.
Then predict_rank alone at the 10 000-target validation shape.  Prints one JSON line; the flops are the
2 n_targets n_anime D of the fp32 chain, the peak the 157.3 TFLOP/s of the fp32 vector units, the times whole calls
(row normalisation and host side included)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops  # noqa: E402

FP32_VALU_PEAK_TFLOPS = 157.3
n_u, n_a, dim = 350_000, 17_560, 128
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
g = torch.Generator(device="cuda")
g.manual_seed(7)
U = torch.randn(n_u, dim, generator=g, device="cuda") * 0.05
A = torch.randn(n_a, dim, generator=g, device="cuda") * 0.05
head = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
ww = (n_a + 31) // 32


def case(n_t):
    users = torch.randperm(n_u, generator=g, device="cuda")[:n_t].to(torch.int32)     # one target per user
    row = torch.arange(n_t, dtype=torch.int32, device="cuda")
    anime = torch.randint(0, n_a, (n_t,), generator=g, device="cuda", dtype=torch.int32)
    w = torch.randint(-2**31, 2**31 - 1, (n_t, ww), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    w &= torch.randint(-2**31, 2**31 - 1, w.shape, generator=g, device="cuda", dtype=torch.int64).to(torch.int32)  # ~25 %
    return users, row, anime, w


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def by_rank(c):
    return ops.predict_rank(U, A, head, c[0], c[1], c[2], c[3])[0]


def by_whole_ranking(c):
    users, row, anime, w = c
    m = w.clone()
    a64 = anime.to(torch.int64)
    word = m[row.to(torch.int64), a64 >> 5]
    m[row.to(torch.int64), a64 >> 5] = word & ~(torch.ones_like(word) << (anime & 31))
    idx, _ = ops.predict_topk(U, A, head, users, n_a, m)
    return (idx == anime[:, None]).to(torch.int32).argmax(1).to(torch.int32)


c = case(4096)
r_new, r_old = by_rank(c), by_whole_ranking(c)          # warm-up of both, and the comparison
same = bool(torch.equal(r_new, r_old))
t_new, t_old = [], []
for _ in range(reps):
    t_new.append(timed(lambda: by_rank(c))[0])
    t_old.append(timed(lambda: by_whole_ranking(c))[0])
v = case(10_000)
by_rank(v)
t_val = [timed(lambda: by_rank(v))[0] for _ in range(reps)]


def med(x):
    return sorted(x)[len(x) // 2]


def tflops(n_t, dt):
    return 2.0 * n_t * n_a * dim / dt / 1e12


print(json.dumps({
    "device": torch.cuda.get_device_name(0), "n_anime": n_a, "dim": dim, "reps": reps, "ranks_equal": same,
    "targets": 4096, "predict_rank_ms": med(t_new) * 1e3, "predict_rank_ms_all": [round(x * 1e3, 3) for x in t_new],
    "whole_ranking_ms": med(t_old) * 1e3, "whole_ranking_ms_all": [round(x * 1e3, 3) for x in t_old],
    "speedup": med(t_old) / med(t_new), "predict_rank_tflops_of_call": tflops(4096, med(t_new)),
    "frac_fp32_valu_peak_of_call": tflops(4096, med(t_new)) / FP32_VALU_PEAK_TFLOPS,
    "validation_targets": 10_000, "validation_ms": med(t_val) * 1e3,
    "validation_ms_all": [round(x * 1e3, 3) for x in t_val],
    "validation_frac_fp32_valu_peak_of_call": tflops(10_000, med(t_val)) / FP32_VALU_PEAK_TFLOPS}))
