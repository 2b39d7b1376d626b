"""The item-kNN from co-occurrence at the full data set's size (arguments: reps), beside a torch route on the same device.

neighbours   all-items top-50 neighbours at 17 560 items x 350 000 users with about 109 M set bits (uniform density; the
             kernels' time does not depend on where the bits lie): ``recs.cooc_neighbours`` (anirec_cooc_scores +
             anirec_rows_topk, 1024 queries a batch) against fp16 0 / 1 ``B @ B.T`` over batches of 2048 users (a partial
             count is then exact in fp16) summed in fp32, the cosine from the counts, the diagonal masked, ``topk``.  The
             torch route's fp16 matrix (12.3 GB) is built before the clock starts.
histories    ``recs.itemknn_topk`` (anirec_itemknn_scores + anirec_rows_topk, top 10) for 10 000 users x 300 history
             entries x K = 50 against ``index_add_`` of the same terms into a zeroed [users, items] fp32 table and ``topk``,
             4096 users a batch on both routes.

Host clock around a device synchronise, after a warm-up of each route; the routes alternate inside every repetition and
the medians are reported.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import recs  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N_ITEMS, N_USERS, SET_BITS, K = 17_560, 350_000, 109_000_000, 50
N_LISTS, HIST, TOP = 10_000, 300, 10
USER_BATCH, LIST_BATCH = 2048, 4096


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def make_bits(g):
    """int32 [N_ITEMS, ceil(N_USERS/32)] liked-by rows and the same matrix as fp16 0 / 1 [N_ITEMS, words * 32]"""
    words = (N_USERS + 31) // 32
    p = SET_BITS / (N_ITEMS * N_USERS)
    bits = torch.empty(N_ITEMS, words, dtype=torch.int32, device="cuda")
    dense = torch.zeros(N_ITEMS, words * 32, dtype=torch.float16, device="cuda")
    weights = (1 << torch.arange(32, device="cuda", dtype=torch.int64))
    for r0 in range(0, N_ITEMS, 256):
        r1 = min(N_ITEMS, r0 + 256)
        m = torch.rand(r1 - r0, words * 32, generator=g, device="cuda") < p
        m[:, N_USERS:] = False
        dense[r0:r1] = m.to(torch.float16)
        w = (m.view(r1 - r0, words, 32).to(torch.int64) * weights).sum(dim=2)
        bits[r0:r1] = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)
    return bits, dense


def torch_neighbours(dense):
    C = torch.zeros(N_ITEMS, N_ITEMS, dtype=torch.float32, device="cuda")
    for u0 in range(0, dense.shape[1], USER_BATCH):
        b = dense[:, u0:u0 + USER_BATCH]
        C += (b @ b.T).float()
    pop = C.diagonal().clone()
    sim = C / (pop[:, None] * pop[None, :]).sqrt().clamp_min(1.0)
    sim.fill_diagonal_(-1.0)
    return torch.topk(sim, K, dim=1)


def neighbours(g):
    bits, dense = make_bits(g)
    ours = lambda: recs.cooc_neighbours(bits, N_USERS, K)
    theirs = lambda: torch_neighbours(dense)
    timed(ours), timed(theirs)                                  # warm-up
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ours)[0])
        b.append(timed(theirs)[0])
    idx, sim, _ = ours()
    tv, ti = theirs()
    words = bits.shape[1]
    ms = median(a)
    return {"n_items": N_ITEMS, "n_users": N_USERS, "set_bits": int(dense.sum(dtype=torch.float32)), "k": K,
            "cooc_neighbours_ms": ms, "torch_ms": median(b), "torch_over_ours": median(b) / ms,
            "word_pairs": N_ITEMS * N_ITEMS * words, "t_lane_ops_per_s": 2 * N_ITEMS * N_ITEMS * words / ms / 1e9,
            "winner": "libanirec" if ms < median(b) else "torch",
            # the two routes break ties differently (index order against topk's) and torch divides in fp32: the best
            # neighbour's similarity agrees to rounding
            "same_best_similarity": float((sim[:, 0] == tv[:, 0]).float().mean()),
            "best_similarity_max_abs_diff": float((sim[:, 0] - tv[:, 0]).abs().max())}


def torch_histories(nbr_idx, nbr_sim, hist):
    out = []
    for l0 in range(0, N_LISTS, LIST_BATCH):
        h = hist[l0:l0 + LIST_BATCH]                            # [lists, HIST]
        n = h.shape[0]
        j = nbr_idx[h].reshape(n, -1).long()                    # [lists, HIST * K]
        v = nbr_sim[h].reshape(n, -1)
        flat = (j + torch.arange(n, device="cuda")[:, None] * N_ITEMS).reshape(-1)
        S = torch.zeros(n * N_ITEMS, dtype=torch.float32, device="cuda").index_add_(0, flat, v.reshape(-1))
        out.append(torch.topk(S.view(n, N_ITEMS), TOP, dim=1))
    return out


def histories(g):
    nbr_idx = torch.randint(0, N_ITEMS, (N_ITEMS, K), generator=g, device="cuda", dtype=torch.int32)
    nbr_sim = torch.rand(N_ITEMS, K, generator=g, device="cuda")
    hist = torch.randint(0, N_ITEMS, (N_LISTS, HIST), generator=g, device="cuda", dtype=torch.int32)
    knn = {"nbr_idx": nbr_idx, "nbr_sim": nbr_sim}
    off = torch.arange(0, (N_LISTS + 1) * HIST, HIST, dtype=torch.int32).numpy()
    flat = hist.reshape(-1)
    ours = lambda: recs.itemknn_topk(knn, off, flat, None, TOP, None, batch=LIST_BATCH)
    theirs = lambda: torch_histories(nbr_idx.long(), nbr_sim, hist.long())
    timed(ours), timed(theirs)
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ours)[0])
        b.append(timed(theirs)[0])
    idx, _ = ours()
    ti = torch.cat([t.indices for t in theirs()])
    ms = median(a)
    return {"n_lists": N_LISTS, "history": HIST, "k_neighbours": K, "top": TOP, "itemknn_topk_ms": ms, "torch_ms": median(b),
            "torch_over_ours": median(b) / ms, "terms_per_s": N_LISTS * HIST * K / ms * 1e3,
            "winner": "libanirec" if ms < median(b) else "torch",
            "same_best_item": float((idx[:, 0].long() == ti[:, 0]).float().mean())}


g = torch.Generator(device="cuda")
g.manual_seed(7)
out = {"device": torch.cuda.get_device_name(0), "reps": reps, "histories": histories(g)}
out["neighbours"] = neighbours(g)
print(json.dumps(out))
