"""ops.group_topk at the serving shapes: 1, 10 000 and 100 000 groups of 4 and 10 000 groups of 16, against 17 560
anime, D = 128, k = 10, mean strategy, under watched bits (1 / 8 of the bits set), members drawn from 100 000 users
(arguments: reps, anime, users).  Beside each the torch route on the same GPU: ``ops.predict_grid`` over the members in
batches (at most 8192 member rows: a 575 MB grid), a torch mean over each group's rows, the union of the members'
watched words, ``torch.topk``.  Host clock around a device synchronise; one warm-up call of each route, then the two
routes alternate and the median of each is reported; whole wrapper calls (allocation of outputs and workspace and the
error-word read-back included).  The two routes' aggregate scores must agree to allclose (the torch mean sums in
another order), and their lists wherever neighbouring scores differ by more than that.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n_a = int(sys.argv[2]) if len(sys.argv) > 2 else 17_560
n_u = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
dim, k = 128, 10
MEMBER_ROWS = 8192
head = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
words = (n_a + 31) // 32

g = torch.Generator(device="cuda")
g.manual_seed(7)
U = torch.randn(n_u, dim, generator=g, device="cuda") * 0.05
A = torch.randn(n_a, dim, generator=g, device="cuda") * 0.05
users = torch.arange(n_u, dtype=torch.int32, device="cuda")


def rand_words():
    return torch.randint(-2 ** 31, 2 ** 31, (n_u, words), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)


watched = rand_words() & rand_words() & rand_words()
shifts = torch.arange(32, device="cuda", dtype=torch.int32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def torch_route(member_row, n_g, c):
    """mean of predict_grid rows, union mask, torch.topk, MEMBER_ROWS member rows at a time"""
    idx = torch.empty(n_g, k, dtype=torch.int64, device="cuda")
    score = torch.empty(n_g, k, dtype=torch.float32, device="cuda")
    per = max(1, MEMBER_ROWS // c)
    for g0 in range(0, n_g, per):
        rows = member_row[g0 * c:(g0 + per) * c]
        b = rows.numel() // c
        P = ops.predict_grid(U, A, head, rows)
        agg = P.view(b, c, n_a).mean(dim=1)
        w = watched[rows.long()].view(b, c, words)
        union = w[:, 0]
        for i in range(1, c):
            union = union | w[:, i]
        seen = ((union.unsqueeze(-1) >> shifts) & 1).view(b, words * 32)[:, :n_a].bool()
        top = torch.topk(agg.masked_fill(seen, float("-inf")), k, dim=1)
        idx[g0:g0 + b], score[g0:g0 + b] = top.indices, top.values
    return idx, score


def shape(n_g, c):
    member_row = torch.randint(0, n_u, (n_g * c,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    offsets = torch.arange(0, n_g * c + 1, c, dtype=torch.int32)

    def ours():
        return ops.group_topk(U, A, head, users, offsets, member_row, k, mode="mean", watched_bits=watched)

    def theirs():
        return torch_route(member_row, n_g, c)

    (gi, gs), (ti, ts) = timed(ours)[1], timed(theirs)[1]     # warm-up, and the comparison
    close = bool(torch.allclose(gs, ts, rtol=0, atol=1e-6))
    t_ours, t_theirs = [], []
    for _ in range(reps):                                       # the two routes alternate
        t_ours.append(timed(ours)[0])
        t_theirs.append(timed(theirs)[0])
    med = lambda t: sorted(t)[len(t) // 2] * 1e3                # noqa: E731
    return {"groups": n_g, "members": c, "group_topk_ms": med(t_ours), "torch_route_ms": med(t_theirs),
            "ratio": med(t_theirs) / med(t_ours), "group_topk_ms_min_max": [min(t_ours) * 1e3, max(t_ours) * 1e3],
            "chain_gfma_per_s": n_g * c * n_a * dim / med(t_ours) / 1e6, "scores_allclose": close,
            "lists_equal_share": float((gi.long() == ti).float().mean())}


shapes = [shape(1, 4), shape(10_000, 4), shape(100_000, 4), shape(10_000, 16)]
assert all(s["scores_allclose"] for s in shapes), shapes
print(json.dumps({"device": torch.cuda.get_device_name(0), "n_users": n_u, "n_anime": n_a, "dim": dim, "k": k,
                  "reps": reps, "shapes": shapes}))
