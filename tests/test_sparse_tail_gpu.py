"""The sparse step and bwd at the rows with many chunks: the lazy update against the dense one, bit for bit.

k_bwd and the sparse half of k_lazy_adam walk the anime table's chunk slots first, and every reader of a chunk table
fetches the count word and the chunk record in one round trip.  Neither may move a bit: the dense update (k_adam walks
the row map, not the chunk grid) is the reference for W, M, V and the scalar state, and the dense engine itself is held
to oracle.anirec_oracle at tests/test_train_edges_gpu.py's bars, which guards the bwd mapping both engines share.

The batches are built by hand so that, in the user table and in the anime table, rows of 1, 2, 5, 6, 32, 33, 34 and 64
chunks occur (run lengths 32 n and 32 n - 1), a row being HEAVY from 6 chunks on (more than one add_chunks<4> batch
behind its first partial), and so that the heavy rows sit where the workgroup -> chunk map has its edges: the first and
the last valid chunk of a table, two first chunks in one workgroup's eight slots, a first chunk in slot 7 (the row's
other chunks belong to the next workgroups), the first workgroup of the grid (which also finishes the step).  Every
property is checked on the host from np.unique of the constructed batches, so a change of the construction cannot
silently drop a case.  One run is eager with run(1) calls (steps whose launches carry no catch-up of a next batch),
one replays the captured graph."""
import functools

import numpy as np
import pytest
import torch

from oracle import anirec_oracle as orc

pytestmark = pytest.mark.gpu
f32 = np.float32
LR = 3e-5
N_U, N_A, B = 5000, 64, 2048
STEPS = 11
LAST = 777                                   # the last batch is short
HEAVY = 6                                    # chunks from which a row takes more than one add_chunks<4> batch
CAP_C = (B + B // 32 + 2 + 3) & ~3           # chunk slots per table (chunk_capacity in csrc/anirec_train.hpp)
SMALL = [32, 31, 64, 63, 160, 159, 192, 191]  # 1, 2, 5 and 6 chunks, full and one short

# per step: {row: run length}; the rest of the batch goes to filler rows (anime: rows 20..59 in turn, at most two chunks
# each; users: single ratings of distinct users)
ANIME = [
    {0: 2048},
    {0: 2047, 63: 1},
    {5: 1088, **{6 + k: n for k, n in enumerate(SMALL)}},
    {5: 1087},
    {5: 1056},
    {5: 1055},
    {5: 1024, 6: 1023},
    None,                                    # no heavy row: 32 ratings on each of the 64 rows
    {0: 192, 1: 192, 2: 96, 3: 224, 63: 200},  # first chunks at slots 0 and 6 of workgroup 0, slot 7 of workgroup 1
    {0: 500},
    {7: 400},
]
USERS = [
    {1000: 1056},
    {1000: 1055},
    {1000: 1024, 1001: 1023},
    {},
    {0: 2048},
    {0: 2047, 4999: 1},
    {2000: 1088, **{2001 + k: n for k, n in enumerate(SMALL)}},
    {},                                      # no heavy row
    {0: 128, 1: 192, 2: 192, 3: 96, 4: 192, 4999: 200},
    {0: 192, 2000: 1087},
    {4999: 300},
]


def _runs(idx):
    """rows, run lengths, chunks per row and the index of each row's first chunk in its table (rows ascending)"""
    rows, cnt = np.unique(idx, return_counts=True)
    nch = (cnt + 31) // 32
    return rows, cnt, nch, np.cumsum(nch) - nch


@functools.lru_cache(maxsize=None)
def _problem():
    rng = np.random.default_rng(20261019)
    counts = np.array([B] * (STEPS - 1) + [LAST])
    ui, ai = [], []
    for s, n in enumerate(counts):
        if ANIME[s] is None:
            a = np.resize(np.arange(N_A), n)
        else:
            a = np.concatenate([np.full(c, r) for r, c in ANIME[s].items()])
            a = np.concatenate([a, np.resize(np.arange(20, 60), n - len(a))])
        u = np.concatenate([np.full(c, r) for r, c in USERS[s].items()] + [np.zeros(0, np.int64)])
        pool = np.setdiff1d(np.arange(100, 4900), list(USERS[s]))
        u = np.concatenate([u, rng.choice(pool, n - len(u), replace=False)])
        assert len(a) == len(u) == n
        ui.append(u.astype(np.int64))
        ai.append(rng.permutation(a).astype(np.int64))
    U = rng.uniform(-0.05, 0.05, (N_U, 128)).astype(f32)
    A = rng.uniform(-0.05, 0.05, (N_A, 128)).astype(f32)
    ui, ai = np.concatenate(ui), np.concatenate(ai)
    t = (rng.integers(0, 11, len(ui)) / 10).astype(f32)
    return U, A, ui, ai, t, np.cumsum(counts) - counts, counts


def _batches():
    U, A, ui, ai, t, starts, counts = _problem()
    return [(ui[s:s + c], ai[s:s + c], t[s:s + c]) for s, c in zip(starts, counts)]


def test_the_batches_hold_every_case():
    """host only: the chunk counts and slot positions the module's docstring promises"""
    want = {(n, full) for n in (1, 2, 5, 6, 32, 33, 34, 64) for full in (True, False)}
    batches = _batches()
    for T, name in ((0, "user"), (1, "anime")):
        kinds, same_wg, slot7, first, last, wg0, next_yes, next_no = set(), 0, 0, 0, 0, 0, 0, 0
        for s, bt in enumerate(batches):
            rows, cnt, nch, c0 = _runs(bt[T])
            assert nch.sum() <= CAP_C
            kinds |= {(int(n), bool(c % 32 == 0)) for n, c in zip(nch, cnt)}
            heavy = nch >= HEAVY
            # the grid's chunk slots: the anime table's first, the users' behind them; eight slots per workgroup
            hw = c0 + (0 if T == 1 else CAP_C)
            wgs = hw[heavy] // 8
            same_wg += len(wgs) != len(set(wgs.tolist()))
            slot7 += int(np.any(hw[heavy] % 8 == 7))
            first += int(heavy[0])
            last += int(heavy[-1])
            wg0 += int(np.any(hw[heavy] < 8))
            if s + 1 < len(batches):
                nxt = np.isin(rows[heavy], batches[s + 1][T])
                next_yes += int(nxt.any())
                next_no += int((~nxt).any())
        assert want <= kinds, (name, sorted(want - kinds))
        assert same_wg and slot7 and first and last and next_yes and next_no, (
            name, same_wg, slot7, first, last, next_yes, next_no)
        if T == 1:      # workgroup 0 (it finishes the step) holds the anime table's first slots
            assert wg0
    quiet = [s for s, bt in enumerate(batches) if all((_runs(bt[T])[2] < HEAVY).all() for T in (0, 1))]
    assert quiet, "no step without a heavy row"
    assert len(batches[-1][0]) == LAST < B


@functools.lru_cache(maxsize=None)
def _oracle():
    U, A, ui, ai, t, starts, counts = _problem()
    st = orc.new_state(U, A, orc.new_head(w=1.2))
    mets = [orc.train_step(st, u, a, r, LR)[0] for u, a, r in _batches()]
    return st, mets


def _run(lazy, plan, use_graph):
    """(W, M, V, state record) after the run; plan: the run() calls' step counts"""
    from anime_recommendations_amd.engine import TrainEngine
    U, A, ui, ai, t, starts, counts = _problem()
    eng = TrainEngine(N_U, N_A, max_batch=B, arena_steps=8, lazy=lazy)
    assert eng.lazy == bool(lazy)
    eng.set_head(w=1.2)
    eng.set_weights(U, A)
    eng.reset_optimizer()
    eng.set_epoch(ui, ai, t, starts, counts, [orc.adam_alpha(LR, i + 1) for i in range(STEPS)])
    s = 0
    for n in plan:
        eng.run(n, use_graph=use_graph, first_step=s)
        s += n
    assert s == STEPS
    eng.synchronize()
    rec = eng.read_state()
    assert int(rec["step_fwd"]) == STEPS
    out = (eng.W.clone(), eng.M.clone(), eng.V.clone(), rec, (eng.rowmap.cpu().numpy() == 0).all())
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _dense():
    return _run(False, [STEPS], False)


def test_dense_update_matches_the_oracle():
    """the reference of the two tests below, and the guard of the bwd mapping (test_train_edges_gpu.py's bars)"""
    U, A, ui, ai, t, starts, counts = _problem()
    st, mets = _oracle()
    W, M, V, rec, rowmap_clear = _dense()
    W, M, V = W.cpu().numpy(), M.cpu().numpy(), V.cpu().numpy()
    assert np.isfinite(W).all() and np.isfinite(M).all() and np.isfinite(V).all() and rowmap_clear
    tol = LR * 2e-3 * STEPS + 1e-9
    np.testing.assert_allclose(W[:N_U], st["U"], atol=tol)
    np.testing.assert_allclose(W[N_U:], st["A"], atol=tol)
    for got, want, what in ((M[:N_U], st["mU"], "mU"), (M[N_U:], st["mA"], "mA"),
                            (V[:N_U], st["vU"], "vU"), (V[N_U:], st["vA"], "vA")):
        np.testing.assert_allclose(got, want, atol=np.abs(want).max() * 1e-4, err_msg=what)
    h = st["head"]
    for k in ("w", "gamma", "beta"):
        assert abs(float(rec[k]) - float(h[k])) < tol, k
    assert abs(float(rec["b"]) - float(h["b"])) <= 2.05 * LR * STEPS
    assert abs(rec["mov_mean"] - h["mov_mean"]) < 1e-6 and abs(rec["mov_var"] - h["mov_var"]) < 1e-6
    assert abs(rec["last_loss"] - mets[-1]["loss"]) < 5e-6


# eager: run(1) calls put steps 2, 3 and 10 in blocks of their own (no next batch in the arena: their head and sparse
# launches carry no catch-up, and a stand-alone catch-up launch precedes them); graph: blocks of 8 and 3
@pytest.mark.parametrize("plan,use_graph", [([2, 1, 1, 6, 1], False), ([STEPS], True)], ids=["eager", "graph"])
def test_lazy_update_is_bitwise_the_dense_update(plan, use_graph):
    dense = _dense()
    lazy = _run(True, plan, use_graph)
    for i, what in enumerate("WMV"):
        x, y = dense[i], lazy[i]
        if not torch.equal(x, y):
            bad = torch.nonzero((x != y).any(1)).flatten()
            raise AssertionError("lazy %s differs from dense in %d rows (first %s), max |diff| %.3e" % (
                what, bad.numel(), bad[:8].tolist(), float((x - y).abs().max())))
    for k in ("w", "b", "gamma", "beta", "adam_m", "adam_v", "mov_mean", "mov_var", "bn_mu", "bn_var", "step_fwd"):
        assert np.array_equal(dense[3][k], lazy[3][k]), k
