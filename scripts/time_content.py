"""The content-based score rows at the full data set's size (arguments: reps), beside two torch routes on the same device.

categorical  17 560 items x about 8 tokens over a vocabulary of 400 (the five categorical columns; token draws with a
             long-tailed document frequency), 10 000 and 100 000 users x 300 history entries: ``ops.content_scores``
             (anirec_content_scores, the LDS form), 4096 users a call, and the whole ``recs.content_topk(k=10)``.
synopsis     the same items x about 50 tokens over a vocabulary of 20 000: the workspace form (the profile's int64 row
             of a list lives in global memory).
torch        the profiles as ``torch.sparse.mm`` of the histories' CSR [users, items] against the dense item rows
             [items, tokens], divided by the weights' sum; the scores as (a) ``torch.sparse.mm`` of the item CSR against
             the profile matrix and (b) the dense ``profiles @ rows.T``; then ``topk``.  4096 users a batch as well.  The
             dense item rows (1.4 GB for the synopsis case) are built before the clock starts.

hipEvent timing on the current stream after a warm-up of each route; the routes alternate inside every repetition and the
medians are reported.  Also stated: the bytes each phase moves (the profile phase reads the histories' item rows, the
score phase streams the whole item CSR once per list and writes the score rows), against the HBM and L2 rates.
Prints one JSON line and saves it as profiles/time_content.json."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anime_recommendations_amd import ops, recs  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N_ITEMS, HIST, TOP, LIST_BATCH = 17_560, 300, 10, 4096
USERS = (10_000, 100_000)
HBM_TBS, L2_TBS = 8.0, 20.0        # MI355X: peak HBM3E rate; an aggregate L2 rate of that order (both nominal)


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


def make_fit(rng, n_tokens, per_item):
    """a unit-length item CSR with Zipf-like token draws (a long-tailed document frequency), ids ascending in a row"""
    p = 1.0 / np.arange(1, n_tokens + 1) ** 0.9
    p /= p.sum()
    lens = np.clip(rng.poisson(per_item, N_ITEMS), 1, None)
    rows = [np.unique(rng.choice(n_tokens, n, p=p)) for n in lens]
    off = np.zeros(N_ITEMS + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    idx = np.concatenate(rows).astype(np.int32)
    w = rng.random(len(idx)) + 0.5
    norm = np.sqrt(np.add.reduceat(w * w, off[:-1]))
    w = (w / np.repeat(norm, np.diff(off))).astype(np.float32)
    return {"tok_offsets": torch.as_tensor(off).cuda(), "tok_idx": torch.as_tensor(idx).cuda(),
            "tok_w": torch.as_tensor(w).cuda(), "n_items": N_ITEMS, "n_tokens": n_tokens}


def ours_scores(fit, off, hist, hw):
    for l0 in range(0, len(off) - 1, LIST_BATCH):
        ops.content_scores(fit["tok_offsets"], fit["tok_idx"], fit["tok_w"], fit["n_tokens"], off[l0:l0 + LIST_BATCH + 1],
                           hist, hw, check=False)


def torch_route(X, D, hist, hw, n_lists, dense_scores):
    out = []
    for l0 in range(0, n_lists, LIST_BATCH):
        n = min(LIST_BATCH, n_lists - l0)
        crow = torch.arange(0, (n + 1) * HIST, HIST, device="cuda", dtype=torch.int64)
        sl = slice(l0 * HIST, (l0 + n) * HIST)
        H = torch.sparse_csr_tensor(crow, hist[sl].long(), hw[sl], size=(n, N_ITEMS))
        P = torch.sparse.mm(H, D) / hw[sl].view(n, HIST).abs().sum(dim=1, keepdim=True)
        S = P @ D.T if dense_scores else torch.sparse.mm(X, P.T.contiguous()).T
        out.append(torch.topk(S, TOP, dim=1))
    return out


def case(rng, n_tokens, per_item, users):
    fit = make_fit(rng, n_tokens, per_item)
    nnz = int(fit["tok_idx"].numel())
    X = torch.sparse_csr_tensor(fit["tok_offsets"], fit["tok_idx"].long(), fit["tok_w"], size=(N_ITEMS, n_tokens))
    D = X.to_dense()
    res = {"n_items": N_ITEMS, "n_tokens": n_tokens, "token_slots": nnz, "history": HIST, "top": TOP,
           "form": "lds" if n_tokens <= ops._lib.load().anirec_content_lds_tokens() else "workspace", "users": {}}
    for n_lists in users:
        hist = torch.as_tensor(rng.integers(0, N_ITEMS, n_lists * HIST).astype(np.int32)).cuda()
        hw = torch.as_tensor((rng.integers(1, 11, n_lists * HIST) / 10.0).astype(np.float32)).cuda()
        off = np.arange(0, (n_lists + 1) * HIST, HIST, dtype=np.int64)
        routes = {"content_scores_ms": lambda: ours_scores(fit, off, hist, hw),
                  "content_topk_ms": lambda: recs.content_topk(fit, off, hist, hw, TOP, batch=LIST_BATCH),
                  "torch_sparse_topk_ms": lambda: torch_route(X, D, hist, hw, n_lists, False),
                  "torch_dense_topk_ms": lambda: torch_route(X, D, hist, hw, n_lists, True)}
        ms = {k: [] for k in routes}
        for fn in routes.values():
            timed(fn)                                           # warm-up
        for _ in range(reps):
            for k, fn in routes.items():
                ms[k].append(timed(fn)[0])
        r = {k: median(v) for k, v in ms.items()}
        idx, _ = recs.content_topk(fit, off, hist, hw, TOP, batch=LIST_BATCH)
        ti = torch.cat([t.indices for t in torch_route(X, D, hist, hw, n_lists, True)])
        best = min(r["torch_sparse_topk_ms"], r["torch_dense_topk_ms"])
        # bytes: the profile phase reads 8 B a slot of every history entry's row; the score phase streams the item CSR
        # (8 B a slot + 8 B an item) once per list and writes 4 B per (list, item)
        profile_b = n_lists * HIST * (nnz / N_ITEMS) * 8
        stream_b = n_lists * (nnz * 8 + N_ITEMS * 8)
        write_b = n_lists * N_ITEMS * 4
        s = r["content_scores_ms"] / 1e3
        r.update({"torch_over_ours_topk": best / r["content_topk_ms"],
                  "winner": "libanirec" if r["content_topk_ms"] < best else "torch",
                  "same_best_item": float((idx[:, 0].long() == ti[:, 0]).float().mean()),
                  "profile_read_bytes": profile_b, "csr_stream_bytes_l2": stream_b, "score_write_bytes_hbm": write_b,
                  "csr_stream_tb_per_s": stream_b / s / 1e12, "score_write_tb_per_s": write_b / s / 1e12,
                  "floor_ms_at_l2_rate": stream_b / (L2_TBS * 1e12) * 1e3,
                  "floor_ms_at_hbm_rate": write_b / (HBM_TBS * 1e12) * 1e3})
        res["users"][str(n_lists)] = r
        del hist, hw
    return res


rng = np.random.default_rng(7)
out = {"device": torch.cuda.get_device_name(0), "reps": reps, "list_batch": LIST_BATCH,
       "nominal_hbm_tb_per_s": HBM_TBS, "nominal_l2_tb_per_s": L2_TBS,
       "categorical": case(rng, 400, 8, USERS)}
out["synopsis"] = case(rng, 20_000, 50, USERS if "--full" in sys.argv else USERS[:1])
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "time_content.json"), "w") as f:
    f.write(line + "\n")
