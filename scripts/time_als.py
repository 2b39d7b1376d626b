"""The ALS kernels at the full data set's shape (arguments: reps): a user half-sweep (350 000 rows x 300 entries against a
17 560-row item table), the item half-sweep over the same entries (17 560 rows, long-tailed lengths up to about
200 000), anirec_als_gram of both tables, and anirec_dot_scores + anirec_rows_topk (k = 10) for 10 000 users, at widths
64 and 128 with cg_steps = 3 — beside the torch route to the same problem on the same device: the explicit normal
equations of every row (G + alpha Yi^T Yi + lambda I, batched ``bmm`` over padded lists in batches that fit, the longest
lists one by one) and ``torch.linalg.solve``; ``Y.T @ Y``; ``X @ Y.T`` and ``topk``.  The torch route solves each row
exactly where the kernel takes three conjugate-gradient steps from a warm start: the same problem, not the same answer
(``median_rel_distance_from_exact`` says how far the kernel's rows are from solved).
Host clock around a device synchronise, after a warm-up of each route; the routes alternate inside every repetition and
the medians are reported.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N_USERS, N_ITEMS, PER_USER, CG, ALPHA, LAM = 350_000, 17_560, 300, 3, 1.0, 0.01
PAD_ELEMS = 1 << 28          # floats of one padded gather of the torch route (1 GiB)
LONG = 8192                  # lists longer than this go one by one in the torch route


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def csr(row, col, n_rows):
    order = torch.sort(row, stable=True)[1]
    off = torch.zeros(n_rows + 1, dtype=torch.int64, device=row.device)
    off[1:] = torch.cumsum(torch.bincount(row, minlength=n_rows), 0)
    return off, col[order].to(torch.int32).contiguous()


def torch_half_sweep(Y, off, idx):
    """every row's normal equations solved exactly; returns X"""
    n, F = off.numel() - 1, Y.shape[1]
    G = Y.T @ Y + LAM * torch.eye(F, device=Y.device)
    Yz = torch.cat([Y, torch.zeros(1, F, device=Y.device)])          # row n_other: the padding
    lens = off[1:] - off[:-1]
    order = torch.argsort(lens, descending=True)
    lens_h = lens[order].tolist()
    X = torch.zeros(n, F, device=Y.device)
    p = 0
    while p < n and lens_h[p] > LONG:                                # the longest lists one by one
        r = int(order[p])
        Yi = Y[idx[off[r]:off[r + 1]].long()]
        X[r] = torch.linalg.solve(G + ALPHA * (Yi.T @ Yi), (1 + ALPHA) * Yi.sum(0))
        p += 1
    while p < n:
        L = max(lens_h[p], 1)
        B = max(1, min(n - p, PAD_ELEMS // (L * F)))
        rows = order[p:p + B]
        pos = off[rows][:, None] + torch.arange(L, device=Y.device)[None, :]
        ok = torch.arange(L, device=Y.device)[None, :] < lens[rows][:, None]
        it = torch.where(ok, idx[pos.clamp(max=idx.numel() - 1)].long(), torch.full_like(pos, Y.shape[0]))
        Yi = Yz[it]                                                  # [B, L, F]
        A = G[None] + ALPHA * torch.bmm(Yi.transpose(1, 2), Yi)
        X[rows] = torch.linalg.solve(A, (1 + ALPHA) * Yi.sum(1))
        p += B
    return X


def half(name, Y, off, idx, X0):
    G = ops.als_gram(Y)

    def ours():
        return ops.als_half_sweep(Y, G, off, idx, X0, LAM, CG, alpha=ALPHA, check=False)

    def theirs():
        return torch_half_sweep(Y, off, idx)
    timed(ours)
    timed(theirs)
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ours)[0])
        b.append(timed(theirs)[0])
    rows, loss, err = ours()
    exact = theirs()
    rel = float(((rows - exact).norm(dim=1) / exact.norm(dim=1).clamp(min=1e-30)).median())
    lens = off[1:] - off[:-1]
    return {"half": name, "n_rows": int(off.numel() - 1), "entries": int(idx.numel()), "longest_list": int(lens.max()),
            "half_sweep_ms": median(a), "torch_solve_ms": median(b), "torch_over_kernel": median(b) / median(a),
            "entries_per_us": idx.numel() * (CG + 2) / median(a) / 1e3, "flag": int(err.item()),
            "median_rel_distance_from_exact": rel}


def width(F):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    w = (torch.arange(N_ITEMS, device="cuda", dtype=torch.float64) + 50.0) ** -0.8      # the most liked item: 0.18 % of the pairs
    cdf = torch.cumsum(w / w.sum(), 0)
    u = torch.rand(N_USERS * PER_USER, generator=g, device="cuda", dtype=torch.float64)
    item = torch.searchsorted(cdf, u).clamp(max=N_ITEMS - 1)
    user = torch.arange(N_USERS, device="cuda").repeat_interleave(PER_USER)
    X = torch.randn(N_USERS, F, generator=g, device="cuda") / F ** 0.5
    Y = torch.randn(N_ITEMS, F, generator=g, device="cuda") / F ** 0.5
    u_off, u_idx = csr(user, item, N_USERS)
    i_off, i_idx = csr(item, user, N_ITEMS)
    out = {"factors": F, "halves": [half("user", Y, u_off, u_idx, X), half("item", X, i_off, i_idx, Y)]}
    del user, item, u
    gram = {}
    for name, T in (("items", Y), ("users", X)):
        timed(lambda: ops.als_gram(T))
        timed(lambda: T.T @ T)
        k = median([timed(lambda: ops.als_gram(T))[0] for _ in range(reps)])
        t32 = median([timed(lambda: T.T @ T)[0] for _ in range(reps)])
        t64 = median([timed(lambda: (T.double().T @ T.double()).float())[0] for _ in range(reps)])
        gram[name] = {"n": int(T.shape[0]), "als_gram_ms": k, "torch_fp32_ms": t32, "torch_fp64_ms": t64}
    out["gram"] = gram
    Q = X[:10_000].contiguous()

    def lists():
        return ops.rows_topk(ops.dot_scores(Q, Y), 10)

    def torch_lists():
        return torch.topk(Q @ Y.T, 10, dim=1)
    timed(lists)
    timed(torch_lists)
    a = median([timed(lists)[0] for _ in range(reps)])
    b = median([timed(torch_lists)[0] for _ in range(reps)])
    out["topk_10000_users"] = {"dot_scores_rows_topk_ms": a, "torch_matmul_topk_ms": b, "torch_over_kernel": b / a}
    return out


print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": reps, "cg_steps": CG, "alpha": ALPHA, "reg": LAM,
                  "widths": [width(64), width(128)]}))
