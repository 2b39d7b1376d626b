"""The onboarding greedy at the full data set's size (arguments: reps), beside two torch routes to the SAME picks on the
same device.

shape        17 560 items x 350 000 users, about 109 M set bits: P(user u rated item i) = min(1, pop_i * act_u) with a
             long-tailed popularity pop_i = 0.6 / (1 + rank_i / 100) (the ranks shuffled over the item index) and a
             log-normal activity act_u (sigma 0.8, mean 1).
ours         ``ops.cover_greedy`` (anirec_cover_greedy): m = 20 and m = 100, depth 1 and depth 3.  ms per call, ms per
             pick (the call over m: init, gain passes, tails and info together), and the bytes of bit rows a pick
             streams (n_items * W * 4) over that time, against the 8 TB/s HBM peak and against the best figures of
             profiles/r04_fill_bw.txt (6.42 TB/s hipMemsetAsync, 5.66 TB/s the best plain kernel).
dense        (a) per pick a fp16 0 / 1 matrix times the open vector: the users in chunks of 2048, so that a chunk's
             count is exact in fp16, the chunks summed in fp32; the picked row updates the levels and the open vector.
             The 12.4 GB matrix is built before the clock starts.
incremental  (b) the gains start at the popularity counts; each pick subtracts one from gain[j] for every j in the
             history of each user the pick closed: an int64 ``index_add_`` over a by-user CSR (built before the clock
             starts).  Exact, and O(nnz) over the whole run instead of O(m * bits).  One host read-back per pick.

All three routes break ties to the lowest index and their picks and gains are asserted equal.  Host clock around a device
synchronise, after a warm-up of each route; the routes alternate inside every repetition and the medians are reported.
Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N_ITEMS, N_USERS = 17_560, 350_000
CHUNK = 2048
RUNS = ((20, 1), (20, 3), (100, 1), (100, 3))
HBM_PEAK, FILL_MEMSET, FILL_KERNEL = 8.0e12, 6.42e12, 5.66e12


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def make_data(g):
    """bits int32 [N_ITEMS, W]; dense fp16 [chunks, N_ITEMS, CHUNK]; the by-item and by-user CSRs of the same pairs"""
    words = (N_USERS + 31) // 32
    chunks = (N_USERS + CHUNK - 1) // CHUNK
    rank = torch.randperm(N_ITEMS, generator=g, device="cuda").double()
    pop = 0.6 / (1.0 + rank / 100.0)
    z = torch.randn(N_USERS, generator=g, device="cuda", dtype=torch.float64)
    act = torch.exp(0.8 * z - 0.32)
    bits = torch.empty(N_ITEMS, words, dtype=torch.int32, device="cuda")
    dense = torch.zeros(chunks, N_ITEMS, CHUNK, dtype=torch.float16, device="cuda")
    weights = (1 << torch.arange(32, device="cuda", dtype=torch.int64))
    pairs = []
    for r0 in range(0, N_ITEMS, 256):
        r1 = min(N_ITEMS, r0 + 256)
        p = (pop[r0:r1, None] * act[None, :]).clamp_(max=1.0).float()
        m = torch.zeros(r1 - r0, chunks * CHUNK, dtype=torch.bool, device="cuda")
        m[:, :N_USERS] = torch.rand(r1 - r0, N_USERS, generator=g, device="cuda") < p
        dense[:, r0:r1] = m.view(r1 - r0, chunks, CHUNK).transpose(0, 1).to(torch.float16)
        w = (m[:, :words * 32].reshape(r1 - r0, words, 32).to(torch.int64) * weights).sum(dim=2)
        bits[r0:r1] = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)
        nz = m.nonzero()
        pairs.append((nz[:, 0] + r0) * N_USERS + nz[:, 1])       # item-major keys, ascending
    key = torch.cat(pairs)
    item, user = key // N_USERS, key % N_USERS
    item_ptr = torch.zeros(N_ITEMS + 1, dtype=torch.int64, device="cuda")
    item_ptr[1:] = torch.bincount(item, minlength=N_ITEMS).cumsum(0)
    by_user = torch.sort(user * N_ITEMS + item).values
    user_ptr = torch.zeros(N_USERS + 1, dtype=torch.int64, device="cuda")
    user_ptr[1:] = torch.bincount(user, minlength=N_USERS).cumsum(0)
    return bits, dense, {"item_ptr": item_ptr.cpu(), "item_users": user, "user_ptr": user_ptr,
                         "user_items": by_user % N_ITEMS, "pop": item_ptr[1:] - item_ptr[:-1]}


def _argmax_low(gain):
    """(index, gain) of the largest gain, ties to the lowest index: one unique int64 key"""
    n = gain.numel()
    key = gain.long() * n + (n - 1 - torch.arange(n, device=gain.device))
    k = key.max()
    return (n - 1) - k % n, k // n


def torch_dense(dense, m, depth):
    chunks = dense.shape[0]
    is_open = torch.zeros(chunks * CHUNK, dtype=torch.float16, device="cuda")
    is_open[:N_USERS] = 1.0
    level = torch.zeros(chunks * CHUNK, dtype=torch.int32, device="cuda")
    taken = torch.zeros(N_ITEMS, dtype=torch.bool, device="cuda")
    pick = torch.full((m,), -1, dtype=torch.int64, device="cuda")
    gains = torch.zeros(m, dtype=torch.int64, device="cuda")
    for p in range(m):
        part = torch.bmm(dense, is_open.view(chunks, CHUNK, 1))              # [chunks, N_ITEMS, 1], exact in fp16
        g = part.float().sum(dim=0).view(-1).long()
        i, gi = _argmax_low(torch.where(taken, torch.full_like(g, -1), g))
        ok = gi > 0
        pick[p], gains[p] = torch.where(ok, i, torch.full_like(i, -1)), gi.clamp(min=0)
        hit = (dense.index_select(1, i.view(1)).view(-1) * is_open).to(torch.int32) * ok
        level += hit
        taken[i] |= ok
        is_open = is_open * (level < depth).to(torch.float16)
    return pick, gains


def torch_incremental(csr, m, depth):
    gain = csr["pop"].clone()
    is_open = torch.ones(N_USERS, dtype=torch.bool, device="cuda")
    level = torch.zeros(N_USERS, dtype=torch.int32, device="cuda")
    pick = torch.full((m,), -1, dtype=torch.int64)
    gains = torch.zeros(m, dtype=torch.int64)
    item_ptr, user_ptr = csr["item_ptr"], csr["user_ptr"]
    for p in range(m):
        i, gi = _argmax_low(gain)
        i, gi = int(i), int(gi)                                              # the host read-back of the pick
        if gi <= 0:
            break
        pick[p], gains[p] = i, gi
        us = csr["item_users"][int(item_ptr[i]):int(item_ptr[i + 1])]
        us = us[is_open[us]]
        level[us] += 1
        closed = us[level[us] >= depth]
        is_open[closed] = False
        lo = user_ptr[closed]
        n = user_ptr[closed + 1] - lo
        start = torch.repeat_interleave(lo - (n.cumsum(0) - n), n)
        idx = start + torch.arange(start.numel(), device="cuda")
        gain.index_add_(0, csr["user_items"][idx], torch.full((idx.numel(),), -1, dtype=torch.int64, device="cuda"))
        gain[i] = -1                                                         # picked: no candidate any more
    return pick.cuda(), gains.cuda()


g = torch.Generator(device="cuda")
g.manual_seed(11)
bits, dense, csr = make_data(g)
words = bits.shape[1]
out = {"device": torch.cuda.get_device_name(0), "reps": reps, "n_items": N_ITEMS, "n_users": N_USERS,
       "set_bits": int(csr["pop"].sum()), "most_rated": int(csr["pop"].max()), "bytes_per_pick": N_ITEMS * words * 4,
       "runs": []}
for m, depth in RUNS:
    routes = {"ours": lambda: ops.cover_greedy(bits, N_USERS, m, depth)[:2],
              "dense": lambda: torch_dense(dense, m, depth),
              "incremental": lambda: torch_incremental(csr, m, depth)}
    ms = {k: [] for k in routes}
    res = {k: timed(fn)[1] for k, fn in routes.items()}                      # warm-up of each, and the picks
    for k in ("dense", "incremental"):
        assert torch.equal(res[k][0], res["ours"][0].long()) and torch.equal(res[k][1], res["ours"][1].long()), (m, depth, k)
    for _ in range(reps):
        for k, fn in routes.items():
            ms[k].append(timed(fn)[0])
    t = {k: median(v) for k, v in ms.items()}
    rate = N_ITEMS * words * 4 * m / (t["ours"] * 1e-3)
    out["runs"].append({"m": m, "depth": depth, "picks_made": int((res["ours"][0] >= 0).sum()),
                        "last_gain": int(res["ours"][1][-1]), "ours_ms": t["ours"], "ours_ms_per_pick": t["ours"] / m,
                        "ours_bytes_per_s": rate, "share_of_hbm_peak": rate / HBM_PEAK,
                        "share_of_fill_memset": rate / FILL_MEMSET, "share_of_fill_kernel": rate / FILL_KERNEL,
                        "dense_ms": t["dense"], "incremental_ms": t["incremental"],
                        "dense_over_ours": t["dense"] / t["ours"], "incremental_over_ours": t["incremental"] / t["ours"],
                        "winner": min(t, key=t.get)})
print(json.dumps(out))
