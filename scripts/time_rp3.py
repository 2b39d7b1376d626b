"""RP3beta at the full data set's size (arguments: [reps] [--n N] [--users U]), beside the routes it is read against.

weighted     the all-items user-weighted co-occurrence with the 100 largest weights of every row kept, 17 560 items x
             350 000 users with about 109 M liked pairs (uniform density; the kernels' time does not depend on where
             the bits lie): ``ops.wcooc_scores`` (anirec_wcooc_scores, the i8 matrix cores) + ``ops.rows_topk``, 1024
             query items a call — ``recs.rp3_fit``'s loop without its preparation.  Beside it ``recs.cooc_neighbours`` on
             the same bits: the unweighted popcount job, of which the only exact route to the same sums without the new
             kernel takes one per weight bit-plane, 14 in all.
torch        the torch route on the same GPU: fp16 ``(B * w) @ B.T`` over batches of 2048 users summed in fp32, the two
             scales, the diagonal masked, ``topk``.  It is not exact (the weight is rounded to fp16, the sums are fp32):
             the fraction of rows whose best neighbour agrees is reported.  Its fp16 matrix (12.3 GB) is built before the
             clock starts.
fit          the whole ``recs.rp3_fit`` from the host rating columns (bits, degrees, weights, the loop, the scale).
lists        ``recs.rp3_topk`` (anirec_itemknn_scores + anirec_rows_topk, top 10) for 10 000 users x 300 history entries
             over the fit's tables.

Host clock around a device synchronise, after a warm-up of each route; the routes alternate inside every repetition and
the medians are reported.  Prints one JSON line and saves it as profiles/time_rp3.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anime_recommendations_amd import ops, recs  # noqa: E402

argv = sys.argv[1:]
opt = {"--n": 17_560, "--users": 350_000}
for name in list(opt):
    if name in argv:
        i = argv.index(name)
        opt[name] = int(argv[i + 1])
        del argv[i:i + 2]
reps = int(argv[0]) if argv else 3
N_ITEMS, N_USERS = opt["--n"], opt["--users"]
SET_BITS = int(109_000_000 * (N_ITEMS * N_USERS) / (17_560 * 350_000))
K, ALPHA, BETA = 100, 1.0, 0.3
N_LISTS, HIST, TOP = 10_000, 300, 10
USER_BATCH = 2048
I8_PEAK = 5.0e15        # dense i8 operations a second, nominal


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def make_bits(g):
    """int32 [N_ITEMS, ceil(N_USERS/32)] liked-by rows, the same matrix as fp16 0 / 1 [N_ITEMS, words * 32], and the
    liked pairs (user, item) as host int32 columns"""
    words = (N_USERS + 31) // 32
    p = SET_BITS / (N_ITEMS * N_USERS)
    bits = torch.empty(N_ITEMS, words, dtype=torch.int32, device="cuda")
    dense = torch.zeros(N_ITEMS, words * 32, dtype=torch.float16, device="cuda")
    weights = (1 << torch.arange(32, device="cuda", dtype=torch.int64))
    users, items = [], []
    for r0 in range(0, N_ITEMS, 256):
        r1 = min(N_ITEMS, r0 + 256)
        m = torch.rand(r1 - r0, words * 32, generator=g, device="cuda") < p
        m[:, N_USERS:] = False
        dense[r0:r1] = m.to(torch.float16)
        w = (m.view(r1 - r0, words, 32).to(torch.int64) * weights).sum(dim=2)
        bits[r0:r1] = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)
        i, u = torch.nonzero(m, as_tuple=True)
        users.append(u.to(torch.int32).cpu().numpy())
        items.append((i + r0).to(torch.int32).cpu().numpy())
    return bits, dense, np.concatenate(users), np.concatenate(items)


def weighted_job(bits, uq, row, col):
    q = torch.arange(N_ITEMS, dtype=torch.int32, device="cuda")
    idx = torch.empty(N_ITEMS, K, dtype=torch.int32, device="cuda")
    sim = torch.empty(N_ITEMS, K, dtype=torch.float32, device="cuda")
    for q0 in range(0, N_ITEMS, recs.COOC_BATCH):
        w, _, ex = ops.wcooc_scores(bits, N_USERS, uq, q[q0:q0 + recs.COOC_BATCH], row, col, excl=True)
        idx[q0:q0 + recs.COOC_BATCH], sim[q0:q0 + recs.COOC_BATCH] = ops.rows_topk(w, K, wbits=ex)
    return idx, sim


def kernel_only(bits, uq, row, col):
    q = torch.arange(N_ITEMS, dtype=torch.int32, device="cuda")
    for q0 in range(0, N_ITEMS, recs.COOC_BATCH):
        ops.wcooc_scores(bits, N_USERS, uq, q[q0:q0 + recs.COOC_BATCH], row, col, excl=True, check=False)


def torch_job(dense, wq, row, col):
    S = torch.zeros(N_ITEMS, N_ITEMS, dtype=torch.float32, device="cuda")
    for u0 in range(0, dense.shape[1], USER_BATCH):
        b = dense[:, u0:u0 + USER_BATCH]
        S += ((b * wq[u0:u0 + USER_BATCH]) @ b.T).float()
    S *= row[:, None]
    S *= col[None, :]
    S.fill_diagonal_(-1.0)
    return torch.topk(S, K, dim=1)


g = torch.Generator(device="cuda")
g.manual_seed(11)
note("building %d x %d bits" % (N_ITEMS, N_USERS))
bits, dense, pair_user, pair_item = make_bits(g)
words = bits.shape[1]
pop = ops.cooc_scores(bits, N_USERS, [0], pop=True)[3]
deg = np.bincount(pair_user, minlength=N_USERS)
user_q = recs.rp3_user_weights(deg, ALPHA)
p = pop.cpu().numpy().astype(np.float64)
row_h, col_h = np.zeros(N_ITEMS), np.zeros(N_ITEMS)
row_h[p > 0], col_h[p > 0] = p[p > 0] ** -ALPHA, p[p > 0] ** -BETA
uq = torch.as_tensor(user_q, device="cuda")
row, col = torch.as_tensor(row_h, device="cuda"), torch.as_tensor(col_h, device="cuda")
wq = torch.zeros(dense.shape[1], dtype=torch.float16, device="cuda")
wq[:N_USERS] = (uq.float() / recs.RP3_MAX_Q).half()
row32, col32 = (row * float(recs.RP3_MAX_Q)).float(), col.float()

ours = lambda: weighted_job(bits, uq, row, col)
kern = lambda: kernel_only(bits, uq, row, col)
counts = lambda: recs.cooc_neighbours(bits, N_USERS, K)
theirs = lambda: torch_job(dense, wq, row32, col32)
note("warm-up")
timed(ours), timed(kern), timed(counts), timed(theirs)
a, ak, c, b = [], [], [], []
for r in range(reps):
    a.append(timed(ours)[0])
    ak.append(timed(kern)[0])
    c.append(timed(counts)[0])
    b.append(timed(theirs)[0])
    note("rep %d: weighted %.1f ms (kernel calls alone %.1f), popcount %.1f, torch %.1f" % (r, a[-1], ak[-1], c[-1], b[-1]))
idx, sim = ours()
tv, ti = theirs()
ms, kms, cms, tms = median(a), median(ak), median(c), median(b)
i8_ops = 2 * 2.0 * N_ITEMS * N_ITEMS * words * 32          # two limbs, a multiply and an add a user
out = {"device": torch.cuda.get_device_name(0), "reps": reps,
       "weighted": {"n_items": N_ITEMS, "n_users": N_USERS, "liked_pairs": int(len(pair_user)), "neighbours": K,
                    "wcooc_topk_ms": ms, "wcooc_calls_ms": kms, "cooc_neighbours_ms": cms, "bit_planes": 14,
                    "bit_plane_route_ms": 14 * cms, "bit_plane_route_over_ours": 14 * cms / ms,
                    "popcount_job_over_ours": cms / ms, "i8_ops": i8_ops, "i8_pop_per_s": i8_ops / kms / 1e12,
                    "i8_floor_ms": i8_ops / I8_PEAK * 1e3, "share_of_i8_peak": i8_ops / I8_PEAK * 1e3 / kms},
       "torch": {"user_batch": USER_BATCH, "torch_ms": tms, "torch_over_ours": tms / ms,
                 "winner": "libanirec" if ms < tms else "torch", "exact": False,
                 "same_best_neighbour": float((idx[:, 0].long() == ti[:, 0]).float().mean())}}
del dense, wq, tv, ti
torch.cuda.empty_cache()

note("fit")
rating = np.ones(len(pair_user), np.float32)
fit_fn = lambda: recs.rp3_fit(pair_user, pair_item, rating, N_USERS, N_ITEMS, 0.0, ALPHA, BETA, K)
timed(fit_fn)
f = []
for r in range(reps):
    ms_fit, fit = timed(fit_fn)
    f.append(ms_fit)
    note("rep %d: fit %.1f ms" % (r, ms_fit))
out["fit"] = {"rp3_fit_ms": median(f), "scale": fit["scale"],
              "same_tables_as_the_loop": bool(torch.equal(fit["nbr_idx"], idx))}

note("lists")
hist = torch.randint(0, N_ITEMS, (N_LISTS, HIST), generator=g, device="cuda", dtype=torch.int32).reshape(-1)
off = np.arange(0, (N_LISTS + 1) * HIST, HIST, dtype=np.int32)
lists = lambda: recs.rp3_topk(fit, off, hist, None, TOP)
timed(lists)
l = [timed(lists)[0] for _ in range(reps)]
out["lists"] = {"n_lists": N_LISTS, "history": HIST, "k_neighbours": K, "top": TOP, "rp3_topk_ms": median(l),
                "terms_per_s": N_LISTS * HIST * K / median(l) * 1e3}
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "time_rp3.json"), "w") as fh:
    fh.write(line + "\n")
