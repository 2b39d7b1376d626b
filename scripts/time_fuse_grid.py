"""The rank grid (``ops.fuse_rank_grid``, anirec_fuse_rank_grid) at the catalogue's size (arguments:
reps), beside the only route there was before it: one ``ops.fuse_rows`` plus one ``ops.rows_rank`` per weight vector.

shape    10 000 rows of 17 560 items with one target each, three systems on scales of their own (time_fuse.py's: a
         rating in (0, 1), a neighbour sum that is +0 for nine items in ten, an unbounded dot product), a tenth of every
         row watched (never the target).
grid     ``recs.hybrid_weight_grid(3, 10)``: equal weights and the 66 compositions of 10, 67 vectors.
runs     rrf and minmax.
grid     one ``ops.fuse_rank_grid`` call: every system's row sorted (rrf) or normalised (minmax) once, then a lane per
         weight vector.
loop     per weight vector ``ops.rows_rank(ops.fuse_rows(rows, w), ...)``: 67 fusions of the same rows.
Equality of the two routes' ranks is asserted before anything is timed.  Host clock around a device synchronise, after a
warm-up of each route; the routes alternate inside every repetition and the medians are reported.  Prints one JSON
line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops, recs  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N, S, C, ROWS, CHUNK, STEPS = 17_560, 3, 60, 10_000, 2_500, 10


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def make_data(nq, g):
    """(rows: three fp32 [nq, N]; watched bits int32 [nq, ceil(N/32)]; one target per row, its bit clear)"""
    rows = [torch.rand(nq, N, generator=g, device="cuda"),
            torch.rand(nq, N, generator=g, device="cuda"),
            torch.randn(nq, N, generator=g, device="cuda") * 3.0]
    target = torch.randint(0, N, (nq,), generator=g, device="cuda")
    words = (N + 31) // 32
    place = (1 << torch.arange(32, device="cuda", dtype=torch.int64))
    bits = torch.empty(nq, words, dtype=torch.int32, device="cuda")
    for r0 in range(0, nq, CHUNK):
        r1 = min(nq, r0 + CHUNK)
        rows[1][r0:r1].masked_fill_(torch.rand(r1 - r0, N, generator=g, device="cuda") < 0.9, 0.0)
        watched = torch.zeros(r1 - r0, words * 32, dtype=torch.bool, device="cuda")
        watched[:, :N] = torch.rand(r1 - r0, N, generator=g, device="cuda") < 0.1
        watched[torch.arange(r1 - r0, device="cuda"), target[r0:r1]] = False
        w = (watched.view(r1 - r0, words, 32).to(torch.int64) * place).sum(dim=2)
        bits[r0:r1] = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)
    return rows, bits, target.to(torch.int32)


g = torch.Generator(device="cuda")
g.manual_seed(23)
rows, bits, target = make_data(ROWS, g)
row = torch.arange(ROWS, dtype=torch.int32, device="cuda")
grid = recs.hybrid_weight_grid(S, STEPS)
vectors = [[float(x) for x in w] for w in grid]
out = {"device": torch.cuda.get_device_name(0), "reps": reps, "rows": ROWS, "targets": ROWS, "n_items": N, "n_sys": S,
       "rrf_c": C, "watched_share": 0.1, "grid_steps": STEPS, "n_w": len(vectors), "runs": []}
for method in ("rrf", "minmax"):
    routes = {"grid": lambda: ops.fuse_rank_grid(rows, grid, method, C, row, target, wbits=bits),
              "loop": lambda: torch.stack([ops.rows_rank(ops.fuse_rows(rows, w, method, C, wbits=bits), row, target, bits)
                                           for w in vectors])}
    res = {k: timed(fn)[1] for k, fn in routes.items()}          # warm-up of each, and the results
    assert torch.equal(res["grid"], res["loop"]), method
    distinct = int(torch.unique(res["grid"], dim=0).shape[0])
    del res
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ms[k].append(timed(fn)[0])
    t = {k: median(v) for k, v in ms.items()}
    out["runs"].append({"method": method, "distinct_rank_rows": distinct,
                        "grid_ms": t["grid"], "grid_ms_min": min(ms["grid"]), "grid_ms_max": max(ms["grid"]),
                        "loop_ms": t["loop"], "loop_ms_min": min(ms["loop"]), "loop_ms_max": max(ms["loop"]),
                        "loop_over_grid": t["loop"] / t["grid"], "winner": min(t, key=t.get),
                        "grid_ns_per_target_item_system_vector": t["grid"] * 1e6 / (float(ROWS) * N * S * len(vectors))})
print(json.dumps(out))
