"""The score-row fusion (``ops.fuse_rows``, anirec_fuse_rows) at the catalogue's size (arguments: reps),
beside the torch route on the same device that reaches the SAME bits.

shape    rows of 17 560 items, three systems on scales of their own: a rating in (0, 1), a neighbour sum that is +0 for
         nine items in ten (mass ties), an unbounded dot product; a tenth of every row watched.  The data holds no NaN,
         no infinity and no -0, so torch may sort the floats themselves (a stable descending sort breaks ties to the lower
         index, as the library does) instead of restating score_key.
runs     10 000 rows under rrf and under minmax; the two rows-per-call extremes, 1 and 100 000, under rrf.
ours     one ``ops.fuse_rows`` call (100 000 rows: one call too).
torch    rrf: per system a stable ``argsort`` of the masked row and an ``argsort`` of that order (the ranks), then
         ``w / (c + 1 + rank)`` and the running sum in fp32, in the library's order; minmax: ``amax`` / ``amin`` of the
         masked row, then the same fp32 steps.  10 000 rows at a time, so that the int64 orders of 100 000 rows fit.
Equality of the two routes' uint32 views is asserted before anything is timed.  Host clock around a device synchronise,
after a warm-up of each route; the routes alternate inside every repetition and the medians are reported.  ``min_bytes``
is what a fusion must move at the least (every system's row read once, the fused row written once); its rate is given
against the 8 TB/s HBM peak as an end-to-end figure, not as a kernel's share of peak.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N, S, C, CHUNK = 17_560, 3, 60, 10_000
WEIGHTS = [1.0, 0.5, 2.0]
RUNS = (("rrf", 10_000), ("minmax", 10_000), ("rrf", 1), ("rrf", 100_000))
HBM_PEAK = 8.0e12


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def make_data(nq, g):
    """(rows: three fp32 [nq, N]; watched bool [nq, N]; its bits int32 [nq, ceil(N/32)])"""
    rows = [torch.rand(nq, N, generator=g, device="cuda"),
            torch.rand(nq, N, generator=g, device="cuda"),
            torch.randn(nq, N, generator=g, device="cuda") * 3.0]
    for r0 in range(0, nq, CHUNK):
        sparse = torch.rand(min(CHUNK, nq - r0), N, generator=g, device="cuda") < 0.9
        rows[1][r0:r0 + CHUNK].masked_fill_(sparse, 0.0)
    words = (N + 31) // 32
    watched = torch.zeros(nq, words * 32, dtype=torch.bool, device="cuda")
    weights = (1 << torch.arange(32, device="cuda", dtype=torch.int64))
    bits = torch.empty(nq, words, dtype=torch.int32, device="cuda")
    for r0 in range(0, nq, CHUNK):
        r1 = min(nq, r0 + CHUNK)
        watched[r0:r1, :N] = torch.rand(r1 - r0, N, generator=g, device="cuda") < 0.1
        w = (watched[r0:r1].view(r1 - r0, words, 32).to(torch.int64) * weights).sum(dim=2)
        bits[r0:r1] = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)
    return rows, watched[:, :N], bits


def torch_rrf(rows, watched):
    out = torch.empty_like(rows[0])
    nan = torch.tensor(float("nan"), device="cuda")
    for r0 in range(0, out.shape[0], CHUNK):
        wt = watched[r0:r0 + CHUNK]
        acc = torch.zeros_like(out[r0:r0 + CHUNK])
        for x, w in zip(rows, WEIGHTS):
            order = torch.argsort(x[r0:r0 + CHUNK].masked_fill(wt, float("-inf")), dim=1, descending=True, stable=True)
            rank = torch.argsort(order, dim=1)
            acc = acc + w / (rank + (C + 1)).to(torch.float32)
        out[r0:r0 + CHUNK] = torch.where(wt, nan, acc)
    return out


def torch_minmax(rows, watched):
    out = torch.empty_like(rows[0])
    nan = torch.tensor(float("nan"), device="cuda")
    for r0 in range(0, out.shape[0], CHUNK):
        wt = watched[r0:r0 + CHUNK]
        acc = torch.zeros_like(out[r0:r0 + CHUNK])
        for x, w in zip(rows, WEIGHTS):
            x = x[r0:r0 + CHUNK]
            hi = x.masked_fill(wt, float("-inf")).amax(dim=1, keepdim=True)
            lo = x.masked_fill(wt, float("inf")).amin(dim=1, keepdim=True)
            span = hi - lo
            v = torch.where(span == 0, torch.zeros_like(x), (x - lo) / span)
            acc = acc + w * v
        out[r0:r0 + CHUNK] = torch.where(wt, nan, acc)
    return out


g = torch.Generator(device="cuda")
g.manual_seed(19)
out = {"device": torch.cuda.get_device_name(0), "reps": reps, "n_items": N, "n_sys": S, "weights": WEIGHTS, "rrf_c": C,
       "watched_share": 0.1, "runs": []}
data = {}
for method, nq in RUNS:
    if nq not in data:
        data.clear()                                             # one size on the device at a time
        torch.cuda.empty_cache()
        data[nq] = make_data(nq, g)
    rows, watched, bits = data[nq]
    routes = {"ours": lambda: ops.fuse_rows(rows, WEIGHTS, method, C, wbits=bits),
              "torch": lambda: (torch_rrf if method == "rrf" else torch_minmax)(rows, watched)}
    res = {k: timed(fn)[1] for k, fn in routes.items()}          # warm-up of each, and the results
    assert torch.equal(res["ours"].view(torch.int32), res["torch"].view(torch.int32)), (method, nq)
    eligible = int((~watched).sum())
    del res
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ms[k].append(timed(fn)[0])
    t = {k: median(v) for k, v in ms.items()}
    min_bytes = (S + 1) * nq * N * 4
    out["runs"].append({"method": method, "rows": nq, "eligible_share": eligible / float(nq * N),
                        "ours_ms": t["ours"], "ours_ms_min": min(ms["ours"]), "ours_ms_max": max(ms["ours"]),
                        "torch_ms": t["torch"], "torch_ms_min": min(ms["torch"]), "torch_ms_max": max(ms["torch"]),
                        "torch_over_ours": t["torch"] / t["ours"], "winner": min(t, key=t.get),
                        "ours_us_per_row_and_system": t["ours"] * 1e3 / (nq * S), "min_bytes": min_bytes,
                        "ours_min_bytes_per_s": min_bytes / (t["ours"] * 1e-3),
                        "ours_min_bytes_share_of_hbm_peak": min_bytes / (t["ours"] * 1e-3) / HBM_PEAK})
print(json.dumps(out))
