"""The bootstrap over users at the full data set's size (arguments: reps), beside a torch route to the same bits on the
same device.

boot_sums    ``ops.boot_sums`` at 100 000 and 350 000 units x 41 columns (4 systems x 10 metrics + the count) x 2000
             replicates, Poisson(1) weights, against torch: the weights from the same hash as int64 tensor arithmetic, 64
             replicates a batch (a [64, n_units] int64 temporary per step of the hash), then an fp64 ``matmul`` with the
             values.  The values are what ``ops.rank_gain_rows`` would give for 1-5 targets a unit, so every sum stays
             below 2**53 and the fp64 route is exact: the script checks that both routes give the same integers.
gain rows    ``ops.rank_gain_rows`` at 1 000 000 targets x 4 systems x 10 metrics over 100 000 units (17 560-rank gain
             tables), targets in random order and sorted by unit, against torch: one gather and one ``index_add_`` per
             column into a zeroed int64 [units, 41] table.

Host clock around a device synchronise, after a warm-up of each route; the routes alternate inside every repetition and
the medians are reported, with the spread (max - min) of each.  A short call is timed several calls a sample.  Prints
one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import ops, recs  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N_COL, N_REP, REP_BATCH = 41, 2000, 64
N_T, N_SYS, N_UNITS_GAIN, N_GAIN, KS = 1_000_000, 4, 100_000, 17_560, (1, 5, 10, 50)
M32 = 0xFFFFFFFF
THR = list(recs.POISSON1_THRESHOLDS)


def timed(fn, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def mix32(x):
    """mix32 on int64 tensors holding uint32 values (a wrapped int64 product keeps its low 32 bits)"""
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & M32
    return x ^ (x >> 16)


def torch_boot_sums(values_f64, keys, seed):
    n_units, n_col = values_f64.shape
    out = torch.empty(N_REP + 1, n_col, dtype=torch.float64, device="cuda")
    out[0] = values_f64.sum(dim=0)
    hk = mix32(((keys.long() & M32) + 0x85ebca6b) & M32)
    for b0 in range(1, N_REP + 1, REP_BATCH):
        b = torch.arange(b0, min(b0 + REP_BATCH, N_REP + 1), device="cuda")
        r = mix32(mix32((seed + 0x9e3779b9 * b) & M32)[:, None] ^ hk[None, :])
        w = torch.zeros(r.shape, dtype=torch.float64, device="cuda")
        for t in THR:
            w += r >= t
        out[b0:b0 + b.numel()] = w @ values_f64
    return out


def boot_case(n_units, g):
    values = torch.randint(0, 3 << 30, (n_units, N_COL), generator=g, device="cuda", dtype=torch.int64)
    values[:, -1] = torch.randint(1, 6, (n_units,), generator=g, device="cuda")
    keys = torch.randperm(n_units, generator=g, device="cuda").to(torch.int32)
    vf = values.to(torch.float64)
    ours = lambda: ops.boot_sums(values, keys, 7, N_REP, THR, check=False)[0]
    theirs = lambda: torch_boot_sums(vf, keys, 7)
    timed(ours), timed(theirs)                                  # warm-up
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ours, 5)[0])
        b.append(timed(theirs)[0])
    same = bool((ours() == theirs().to(torch.int64)).all())
    ms = median(a)
    pairs = n_units * (N_REP + 1)
    return {"n_units": n_units, "n_col": N_COL, "n_rep": N_REP, "boot_sums_ms": ms, "boot_sums_spread_ms": max(a) - min(a),
            "torch_ms": median(b), "torch_spread_ms": max(b) - min(b), "torch_over_ours": median(b) / ms,
            "winner": "libanirec" if ms < median(b) else "torch", "same_integers": same,
            "g_pairs_per_s": pairs / ms / 1e6, "g_multiply_adds_per_s": pairs * N_COL / ms / 1e6,
            "value_bytes_read_once": n_units * N_COL * 8}


def torch_gain_rows(ranks, unit, tables, n_units):
    n_metric = tables.shape[0]
    out = torch.zeros(n_units, N_SYS * n_metric + 1, dtype=torch.int64, device="cuda")
    for s in range(N_SYS):
        for m in range(n_metric):
            out[:, s * n_metric + m].index_add_(0, unit, tables[m][ranks[s]])
    out[:, -1].index_add_(0, unit, torch.ones_like(unit))
    return out


def gain_case(g):
    tables = torch.as_tensor(recs.rank_gain_tables(KS, N_GAIN)[0].astype("int64"), device="cuda")
    ranks = torch.randint(0, N_GAIN, (N_SYS, N_T), generator=g, device="cuda", dtype=torch.int32)
    unit = torch.randint(0, N_UNITS_GAIN, (N_T,), generator=g, device="cuda", dtype=torch.int32)
    out = {"n_targets": N_T, "n_sys": N_SYS, "n_metric": int(tables.shape[0]), "n_units": N_UNITS_GAIN, "n_gain": N_GAIN}
    for name, order in (("random_order", None), ("sorted_by_unit", torch.argsort(unit))):
        rk, un = (ranks, unit) if order is None else (ranks[:, order].contiguous(), unit[order].contiguous())
        rl, ul = rk.long(), un.long()
        ours = lambda: ops.rank_gain_rows(rk, un, N_UNITS_GAIN, tables, check=False)[0]
        theirs = lambda: torch_gain_rows(rl, ul, tables, N_UNITS_GAIN)
        timed(ours), timed(theirs)
        a, b = [], []
        for _ in range(reps):
            a.append(timed(ours, 10)[0])
            b.append(timed(theirs)[0])
        ms = median(a)
        out[name] = {"rank_gain_rows_ms": ms, "rank_gain_rows_spread_ms": max(a) - min(a), "torch_ms": median(b),
                     "torch_spread_ms": max(b) - min(b), "torch_over_ours": median(b) / ms,
                     "winner": "libanirec" if ms < median(b) else "torch", "same_integers": bool((ours() == theirs()).all()),
                     "g_gains_per_s": N_T * N_SYS * int(tables.shape[0]) / ms / 1e6}
    return out


g = torch.Generator(device="cuda")
g.manual_seed(7)
out = {"device": torch.cuda.get_device_name(0), "reps": reps, "gain_rows": gain_case(g),
       "boot_sums": [boot_case(n, g) for n in (100_000, 350_000)]}
print(json.dumps(out))
