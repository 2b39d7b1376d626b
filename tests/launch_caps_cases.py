"""The shapes, inputs and references of the launch-cap tests (DESIGN.md "Launch caps"): every case sits just past the
point where a capped grid makes a workgroup take a second pass, or a split call makes a second launch.  A plain helper
module, imported by tests/test_launch_caps_cpu.py and tests/test_launch_caps_gpu.py the way ``bpr_restatement`` is.

The caps are READ from the kernels' source text (``caps()``), so a change that moves one fails the CPU test that holds
each shape against it instead of silently turning these cases back into one-pass cases.  Everything here runs without a
device; a reference is computed once (``lru_cache``) and handed out read-only.
"""
import functools
import os
import re

import numpy as np

import bpr_restatement as B
import cooc_restatement as CO
import rp3_restatement as RP
import tsne_restatement as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anime_recommendations_amd", "csrc")
F32 = np.float32


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(name, pattern):
    """the integer the one match of ``pattern`` in the source file captures"""
    found = re.findall(pattern, _source(name))
    assert len(found) == 1, (name, pattern, found)
    return int(found[0])


def _flat_blocks():
    """k_adam_flat and k_opt_flat: one cap, stated twice"""
    found = set(re.findall(r"if \(blocks > (\d+)\) blocks = \1;\n(?:  hipStream_t s = [^\n]*\n  if [^\n]*\n)?  +hipLaunchKernelGGL\(k_(?:adam|opt)_flat",
                           _source("anirec_train_util.hip")))
    assert len(found) == 1, found
    return int(found.pop())


@functools.lru_cache(maxsize=None)
def caps():
    """the launch caps as the sources state them today"""
    c = dict(
        bpr_blocks=_one("anirec_bpr.hip", r"constexpr int kBprBlocks = (\d+);"),
        bpr_lanes=_one("anirec_bpr.hip", r"constexpr int kNG = (\d+) / kD;"),
        bpr_sample_blocks=_one("anirec_bpr.hip", r"blocks > (\d+) \? \1 : blocks"),
        km_grid=_one("anirec_kmeans.hip", r"constexpr int kKmMaxGrid = (\d+);"),
        km_threads=_one("anirec_kmeans.hip", r"constexpr int kKmThreads = (\d+);"),
        km_image=_one("anirec_kmeans.hip", r"constexpr int kKmImageFloats = (\d+);"),
        km_two_lanes_above=_one("anirec_kmeans.hip", r"constexpr int kL = kD > (\d+) \? 2 : 1;"),
        cooc_tiles=_one("anirec_cooc.hip", r"y0 \+= (\d+)u\)"),
        cooc_tile=_one("anirec_cooc.hip", r"constexpr int kCoocTile = (\d+);"),
        wcooc_tiles=_one("anirec_wcooc.hip", r"y0 \+= (\d+)u\)"),
        wcooc_tile=_one("anirec_wcooc.hip", r"constexpr int kWTile = (\d+);"),
        tsne_init_blocks=_one("anirec_tsne.hip", r"b < (\d+) \? b : \1\)"),
        tsne_threads=_one("anirec_tsne.hip", r"constexpr int kTsThreads = (\d+);"),
        ing_minmax_blocks=_one("anirec_ingest.hip", r"k_ing_minmax, dim3\(g > (\d+) \? \1 : g\)"),
        ing_id_max_blocks=_one("anirec_ingest.hip", r"k_ing_id_max, dim3\(\(unsigned\)\(want > (\d+) \? \1 : want\)\)"),
        ing_id_max_rows=_one("anirec_ingest.hip", r"const int64_t want = \(n \+ \d+\) / (\d+);"),
        ing_rows_blocks=_one("anirec_ingest.hip", r"if \(b > (\d+)\) b = \1;"),
        ing_list_blocks=_one("anirec_ingest.hip", r"const int gl = (\d+);"),
        boot_blocks=_one("anirec_boot.hip", r"blocks > (\d+) \? \1 : blocks"),
        boot_target=_one("anirec_boot.hip", r"constexpr int kBootBlocks = (\d+);"),
        boot_tile=_one("anirec_boot.hip", r"constexpr int kBootTile = (\d+);"),
        boot_col_wide=_one("anirec_boot.hip", r"constexpr int kBootColWide = (\d+);"),
        boot_col_narrow=_one("anirec_boot.hip", r"constexpr int kBootColNarrow = (\d+);"),
        cover_groups=_one("anirec_cover.hip", r"constexpr int kCovMaxGroups = (\d+);"),
        cover_threads=_one("anirec_cover.hip", r"constexpr int kCovThreads = (\d+);"),
        ease_rows=_one("anirec_ease.hip", r"gy = n < (\d+) \? \(unsigned\)n : \1u;"),
        merge_blocks=_one("anirec_infer.hip", r"if \(bx > (\d+)\) bx = \1;"),
        rec_blocks=_one("anirec_recs.hip", r"if \(b > (\d+)\) b = \1;"),
        flat_blocks=_flat_blocks(),
        gather_blocks=_one("anirec_train_util.hip", r"if \(blocks > (\d+)\) blocks = \1;\n  hipLaunchKernelGGL\(k_gather_ratings"),
        rownorm_blocks=_one("anirec_infer.hip", r"if \(blocks > (\d+)\) blocks = \1;"),
        rownorm_floats=_one("anirec_infer.hip", r"int blocks = \(int\)\(\(\(long long\)n \* dim \+ \d+\) / (\d+)\);"),
    )
    init = set(re.findall(r"\(most \+ 255\) / 256 > (\d+) \? \1 : \(most \+ 255\) / 256", _source("anirec_ingest.hip")))
    assert len(init) == 1, init                                  # k_ing_init and k_enc_init: one cap, stated twice
    c["ing_init_blocks"] = int(init.pop())
    return c


def passes(n, per_pass):
    """the passes the busiest workgroup makes over ``n`` elements when one pass of the whole grid covers ``per_pass``"""
    return -(-int(n) // int(per_pass))


# ---- BPR steps --------------------------------------------------------------------------------------------------------
BPR_USERS, BPR_ITEMS = 600, 900
BPR_STEPS = dict(tries=8, seed=11, step0=3, n_steps=2, lr=0.05, reg=0.01, bias=1)
# (width, batch): a third, partial pass at 256; one slot past two passes' start at 128; 33 slots into a second pass at 32
BPR_CASES = ((256, 2 * 16384 + 5), (32, 131072 + 33), (128, 32768 + 1))


def bpr_pass_slots(width):
    """the slots one pass of the capped grid covers at ``width``"""
    c = caps()
    return c["bpr_blocks"] * (c["bpr_lanes"] // width)


@functools.lru_cache(maxsize=None)
def bpr_lists():
    """(offsets, idx, pair_user): 600 users x 900 items, lists of 1 .. 60 items"""
    rng = np.random.default_rng(77)
    lens = rng.integers(1, 61, BPR_USERS)
    lens[:3] = (1, 60, 2)
    u = np.concatenate([np.full(n, r) for r, n in enumerate(lens)])
    i = np.concatenate([np.sort(rng.choice(BPR_ITEMS, n, replace=False)) for n in lens])
    csr = B.csr(u, i, BPR_USERS, BPR_ITEMS)
    for a in csr:
        a.setflags(write=False)
    return csr


@functools.lru_cache(maxsize=None)
def bpr_tables(width):
    rng = np.random.default_rng(9000 + width)
    X = (rng.standard_normal((BPR_USERS, width)) * 0.3).astype(F32)
    Y = (rng.standard_normal((BPR_ITEMS, width)) * 0.3).astype(F32)
    X[:, -1] = 1.0
    X.setflags(write=False), Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def bpr_ref(width, batch):
    """(X', Y', counts, flag) of the restatement for the case, read-only"""
    X, Y = bpr_tables(width)
    p = BPR_STEPS
    out = B.steps(X, Y, *bpr_lists(), batch, p["tries"], p["seed"], p["step0"], p["n_steps"], p["lr"], p["reg"], p["bias"])
    for a in out[:3]:
        a.setflags(write=False)
    return out


def bpr_shared_rows(width, batch, step):
    """(the kept slots of the passes after the first, how many of them touch a row a first-pass slot touched too, how many
    of their row touches, three a slot, fall on such a row): the rows whose count one pass must find exchanged to 0 by
    the other"""
    p = BPR_STEPS
    off, idx, pu = bpr_lists()
    trip = B.sample(off, idx, pu, BPR_ITEMS, batch, p["tries"], p["seed"], p["step0"] + step, 1)[0]
    first = bpr_pass_slots(width)
    kept = trip[:, 2] >= 0
    a, b = trip[:first][kept[:first]], trip[first:][kept[first:]]
    shared = np.stack([np.isin(b[:, 0], a[:, 0]), np.isin(b[:, 1], a[:, 1:]), np.isin(b[:, 2], a[:, 1:])], axis=1)
    return len(b), int(shared.any(axis=1).sum()), int(shared.sum())


# a later pass's OWN rows: on the table above every row a later slot touches was touched by a first-pass slot too, and
# the first-pass winner of the count applies the whole sum, so k_bpr_apply's later passes have nothing left to do.  On
# 200 000 users with one to three items each most later slots touch a user row no first-pass slot touched: the update
# of that row is the later pass's.  Width 64: the width recs.bpr_fit's default batch strides at.
BPR_SPARSE = dict(width=64, batch=65536 + 300, n_users=200_000, n_items=900, tries=8, seed=13, step0=0, n_steps=1, lr=0.05,
                  reg=0.01, bias=1)


@functools.lru_cache(maxsize=None)
def bpr_sparse_lists():
    p = BPR_SPARSE
    rng = np.random.default_rng(78)
    u = np.repeat(np.arange(p["n_users"]), rng.integers(1, 4, p["n_users"]))
    csr = B.csr(u, rng.integers(0, p["n_items"], len(u)), p["n_users"], p["n_items"])
    for a in csr:
        a.setflags(write=False)
    return csr


@functools.lru_cache(maxsize=None)
def bpr_sparse_tables():
    p = BPR_SPARSE
    rng = np.random.default_rng(9064)
    X = (rng.standard_normal((p["n_users"], p["width"]), dtype=F32) * F32(0.3)).astype(F32)
    Y = (rng.standard_normal((p["n_items"], p["width"]), dtype=F32) * F32(0.3)).astype(F32)
    X[:, -1] = 1.0
    X.setflags(write=False), Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def bpr_sparse_ref():
    """(X', Y', counts, flag) of the restatement, and the user rows only slots of the later pass touch"""
    p = BPR_SPARSE
    csr = bpr_sparse_lists()
    out = B.steps(*bpr_sparse_tables(), *csr, p["batch"], p["tries"], p["seed"], p["step0"], p["n_steps"], p["lr"], p["reg"],
                  p["bias"])
    trip = B.sample(*csr, p["n_items"], p["batch"], p["tries"], p["seed"], p["step0"], 1)[0]
    first = bpr_pass_slots(p["width"])
    kept = trip[:, 2] >= 0
    own = np.setdiff1d(trip[first:][kept[first:], 0], trip[:first][kept[:first], 0])
    for a in out[:3] + (own,):
        a.setflags(write=False)
    return out + (own,)


# ---- BPR sampler ------------------------------------------------------------------------------------------------------
SAMPLE = dict(batch=1 << 20, tries=8, seed=5, step0=2, n_steps=17)
SAMPLE_CHECKED = (0, 15, 16)     # step 15 straddles the first pass's end, step 16 lies wholly past it


def sample_pass_entries():
    return caps()["bpr_sample_blocks"] * 256


@functools.lru_cache(maxsize=None)
def sample_ref(step):
    """int32 [batch, 3]: the triples of step ``step`` of the case, by the restatement called for that step alone"""
    p = SAMPLE
    out = B.sample(*bpr_lists(), BPR_ITEMS, p["batch"], p["tries"], p["seed"], p["step0"] + step, 1)[0]
    out.setflags(write=False)
    return out


# ---- k-means ----------------------------------------------------------------------------------------------------------
KM_A = dict(dim=32, k=3, n_rows=262144 + 300)                    # one tile: the image staged once, reused on the second batch
KM_B = dict(dim=256, k=128 + 1, n_rows=131072 + 129)             # tile + 1 centroids: restaged on the second batch
KM_FIT_ITERS = 2


def km_tile(dim):
    return caps()["km_image"] // dim


def km_pass_rows(dim):
    """the rows one pass of the capped grid covers: two lanes share a row above width 128"""
    c = caps()
    return c["km_grid"] * (c["km_threads"] // (2 if dim > c["km_two_lanes_above"] else 1))


def km_planted(case):
    """(the unusable row, twin A, twin B): all inside the second pass, the twins in different workgroups' batches where the
    pass has two"""
    first = km_pass_rows(case["dim"])
    return first + 7, first + 20, case["n_rows"] - 1


# ---- co-occurrence ----------------------------------------------------------------------------------------------------
COOC = dict(n_items=5, n_users=40, nq=32768 * 64 + 70, bad_query=7, measure="cosine", shrink=0.5, min_support=2)
COOC_BAD_AT = COOC["nq"] - 3                                      # in the partial last tile of the second launch


@functools.lru_cache(maxsize=None)
def cooc_inputs():
    """(bits uint32 [5, 2], queries int32 [nq]: the items in a cycle and one query out of range, row int64 [nq]: the row
    of the six distinct queries' oracle that belongs to each query, user_q int32 [40], row_scale, col_scale fp64 [5])"""
    rng = np.random.default_rng(31)
    n, m = COOC["n_items"], COOC["n_users"]
    L = rng.random((n, m)) < 0.4
    L[0, :2], L[1, :2] = True, True                              # a pair above the support for certain
    L[4, :] = False
    L[4, 39] = True                                              # an item of one user: below the support against all
    bits = CO.pack_bits(L)
    row = np.arange(COOC["nq"], dtype=np.int64) % n
    row[COOC_BAD_AT] = n
    queries = row.astype(np.int32)
    queries[COOC_BAD_AT] = COOC["bad_query"]
    user_q = rng.integers(0, RP.MAX_Q + 1, m).astype(np.int32)
    rs, cs = rng.random(n) + 0.5, rng.random(n) * 1e-3 + 1e-4
    for a in (bits, queries, row, user_q, rs, cs):
        a.setflags(write=False)
    return bits, queries, row, user_q, rs, cs


def cooc_distinct():
    """the six distinct queries: the five items and the one out of range"""
    return np.array(list(range(COOC["n_items"])) + [COOC["bad_query"]], np.int32)


@functools.lru_cache(maxsize=None)
def cooc_ref():
    """(sim [6, 5], count, excl, pop, flag) of cooc_restatement.cooc_scores on the six distinct queries"""
    bits = cooc_inputs()[0]
    return CO.cooc_scores(bits, COOC["n_users"], cooc_distinct(), CO.COSINE, COOC["shrink"], COOC["min_support"])


@functools.lru_cache(maxsize=None)
def wcooc_ref():
    """(w [6, 5], sum, excl, flag) of rp3_restatement.wcooc_scores on the six distinct queries"""
    bits, _, _, user_q, rs, cs = cooc_inputs()
    return RP.wcooc_scores(bits, COOC["n_users"], user_q, cooc_distinct(), rs, cs)


def cooc_tile_rows(tile):
    """the query indices of tile ``tile`` (of 64 queries) of the case"""
    t = caps()["cooc_tile"]
    return slice(tile * t, min((tile + 1) * t, COOC["nq"]))


# ---- t-SNE ------------------------------------------------------------------------------------------------------------
TSNE = dict(n=262144 + 200, cluster=50, first=262144 + 100, spacing=2.0 ** 17, exag_iters=2, exaggeration=12.0, lr=20.0)
TSNE_ITERS = (1, 3)


@functools.lru_cache(maxsize=None)
def tsne_case():
    """(Y fp32 [n, 2], offsets int64 [n + 1], idx int32, val fp32, cluster rows, (offsets, idx, val) of the 50 alone).

    Every row but 50 sits on a lattice of spacing 2^17 that starts one spacing away from the origin; the 50 sit around
    the origin (N(0, 1) * 2) at rows 262 244 .. 262 293, past the first pass of k_tsne_init, with stored pairs among
    themselves only.

    Why the lattice adds exactly 0 to every sum: any pair with a lattice point in it is at least 2^17 - 16 > 2^16.9
    apart (the 50 stay inside |y| < 16, asserted where they move), so d2 >= 2^33.8, q = 1 / (1 + d2) <= 2^-33.8 and
    q 2^30 <= 2^-3.8 < 1/2: I(q) = 0.  |dx| < 2^27, so w |dx| = q^2 |dx| < 2^-40 and I(w dx) = 0 likewise.  The fp32
    roundings of the chain move each value by 2^-23 relative, nowhere near the 1/2 that rint needs.  So the rows of the
    50 have the sums of the 50 alone, Z is the 50's, and a lattice row has sums of 0 (it stores no pair)."""
    p = TSNE
    n, m, first = p["n"], p["cluster"], p["first"]
    rng = np.random.default_rng(4242)
    rows = np.arange(first, first + m)
    Y = np.empty((n, 2), F32)
    lat = np.setdiff1d(np.arange(n), rows)
    t = np.arange(len(lat))
    Y[lat, 0] = ((1 + t // 512) * p["spacing"]).astype(F32)
    Y[lat, 1] = ((t % 512) * p["spacing"]).astype(F32)
    Yc = (rng.standard_normal((m, 2)) * 2).astype(F32)
    Y[rows] = Yc
    P = np.triu((rng.random((m, m)) < 0.3) * (rng.random((m, m)) * 0.25 + 0.01), 1)
    P = (P + P.T).astype(F32)
    off50, idx50, val50 = TS.csr_from_dense(P)
    offsets = np.zeros(n + 1, np.int64)
    offsets[first + 1:first + m + 1] = off50[1:]
    offsets[first + m + 1:] = off50[-1]
    idx = (idx50.astype(np.int64) + first).astype(np.int32)
    for a in (Y, offsets, idx, val50, off50, idx50):
        a.setflags(write=False)
    return Y, offsets, idx, val50, rows, (off50, idx50, val50)


def _tsne_cluster_forces(Yc, sub):
    assert (np.abs(Yc) < 16).all()                               # the bound the lattice's zeros rest on
    return TS.forces(Yc, *sub)


@functools.lru_cache(maxsize=None)
def tsne_forces_ref():
    """(Rx, Ry, Ax, Ay int64 [n], Z, info): the 50's own sums at their rows, 0 elsewhere"""
    Y, _, _, _, rows, sub = tsne_case()
    rx, ry, ax, ay, Z, info = _tsne_cluster_forces(Y[rows], sub)
    full = []
    for v in (rx, ry, ax, ay):
        f = np.zeros(len(Y), np.int64)
        f[rows] = v
        f.setflags(write=False)
        full.append(f)
    return tuple(full) + (Z, info)


def tsne_lattice_probe():
    """the restatement on the 50 and the two lattice points nearest to them: (the sums of the 52, the sums of the 50
    alone).  The lattice rows must come out 0 and the 50's rows and Z unchanged."""
    Y, _, _, _, rows, sub = tsne_case()
    near = np.array([[TSNE["spacing"], 0.0], [TSNE["spacing"], TSNE["spacing"]]], F32)
    assert all((Y == q).all(axis=1).any() for q in near)         # both are rows of the case
    off = np.concatenate([sub[0], [sub[0][-1]] * 2])
    return TS.forces(np.concatenate([Y[rows], near]), off, sub[1], sub[2]), TS.forces(Y[rows], *sub)


@functools.lru_cache(maxsize=None)
def tsne_fit_ref(iters):
    """(Y fp32 [n, 2], V, G fp64 [n, 2], info) after ``iters`` iterations: the forces of the 50 alone each iteration (the
    lattice adds 0, see ``tsne_case``), then the restatement's update of ALL n rows — the update divides by n, so the
    50 cannot be fitted as a table of their own"""
    p = TSNE
    Y0, _, _, _, rows, sub = tsne_case()
    Y = Y0.copy()
    n = len(Y)
    V, G = np.zeros((n, 2), np.float64), np.ones((n, 2), np.float64)
    info = 0
    for t in range(iters):
        rx, ry, ax, ay, Z, bits = _tsne_cluster_forces(Y[rows], sub)
        info |= bits
        sums = []
        for v in (rx, ry, ax, ay):
            f = np.zeros(n, np.int64)
            f[rows] = v
            sums.append(f)
        early = t < p["exag_iters"]
        Y, V, G = TS.update(Y, V, G, *sums, Z, p["exaggeration"] if early else 1.0, 0.5 if early else 0.8, p["lr"])
    assert (np.abs(Y[rows]) < 16).all()
    for a in (Y, V, G):
        a.setflags(write=False)
    return Y, V, G, info


# ---- ingest -----------------------------------------------------------------------------------------------------------
INGEST_ROWS = 600_000
INGEST_USER_SCALE = 150          # the frame's user ids (below 4500) spread out past k_ing_init's first pass
INGEST_LIST_ROWS = 1_150_000     # ungrouped rows: every complete row is on the list the k_nl_* kernels stride over
INGEST_ENCODE_IDS = 200_000     # distinct ids (times 3, plus 1) of the encode case: a bound past k_enc_init's first pass
ID_MAX_ROWS = 2048 * 4096 + 7    # k_ing_id_max: 4096 rows a workgroup pass (256 lanes x 4 quads of 4 rows)


# ---- rownorm, bootstrap weights ---------------------------------------------------------------------------------------
ROWNORM_WIDTHS = (32, 256)
BOOT_WEIGHTS = dict(n_units=4097, n_rep=4096)    # 4096 entries past the 16 777 216 of one pass


def rownorm_pass_rows(dim):
    c = caps()
    return c["rownorm_blocks"] * (c["rownorm_floats"] // dim)


# ---- the flat optimiser steps, the rating gather ----------------------------------------------------------------------
FLAT_ELEMS = 4096 * 256 + 77
GATHER_ROWS = 8192 * 256 + 33


# ---- bootstrap sums, onboarding lists, EASE weights -------------------------------------------------------------------
BOOT_SPLITS = dict(n_units=1224, n_col=25, n_rep=16383)      # 8 splits over 10 unit tiles
BOOT_COMBINE = dict(n_units=3, n_col=256, n_rep=65536)       # 65 537 x 256 cells: 256 past one pass of k_boot_combine
COVER_ITEMS = 768 * 8 + 9
EASE_ROWS = 1024 + 5


def boot_splits(n_units, n_col, n_rep):
    """(the unit splits of a call as anirec_boot.hip's boot_splits states them, the unit tiles)"""
    c = caps()
    rep_blocks = (n_rep + 1 + 255) // 256
    ct = c["boot_col_narrow"] if n_col <= c["boot_col_narrow"] else c["boot_col_wide"]
    per = rep_blocks * (-(-n_col // ct))
    tiles = -(-n_units // c["boot_tile"])
    return max(1, min(-(-c["boot_target"] // per), tiles, 65535)), tiles


def cover_pass_items():
    """the items one pass of k_cover_gain's grid holds: a wave a row"""
    c = caps()
    return c["cover_groups"] * (c["cover_threads"] // 64)


# ---- the any-k select's merge, the favourites' scatter ----------------------------------------------------------------
MERGE_COLS = 4096 * 256 + 4099
SCATTER_ROWS = 16384 * 256 + 4099
