"""ops.score_rank (the popularity baseline's ranks) at 10 000 targets x 17 560 anime, one target per user, ~25 % of the
watched bits set, integer scores with many ties: whole calls after a warm-up, host clock around a device synchronise
(as time_rank.py).  Prints one JSON line; a call makes n_targets x n_anime key comparisons."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops  # noqa: E402

n_t, n_a = 10_000, 17_560
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
g = torch.Generator(device="cuda")
g.manual_seed(7)
score = torch.randint(0, 3000, (n_a,), generator=g, device="cuda").to(torch.float32)
row = torch.arange(n_t, dtype=torch.int32, device="cuda")
anime = torch.randint(0, n_a, (n_t,), generator=g, device="cuda", dtype=torch.int32)
ww = (n_a + 31) // 32
w = torch.randint(-2**31, 2**31 - 1, (n_t, ww), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
w &= torch.randint(-2**31, 2**31 - 1, w.shape, generator=g, device="cuda", dtype=torch.int64).to(torch.int32)  # ~25 %


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


call = lambda: ops.score_rank(score, n_t, row, anime, w)
first = call()
again = call()
t = sorted(timed(call)[0] for _ in range(reps))
print(json.dumps({"device": torch.cuda.get_device_name(0), "targets": n_t, "n_anime": n_a, "reps": reps,
                  "identical_bytes": bool(torch.equal(first, again)), "score_rank_ms": t[len(t) // 2] * 1e3,
                  "score_rank_ms_all": [round(x * 1e3, 3) for x in t],
                  "compares_per_s": n_t * n_a / t[len(t) // 2]}))
