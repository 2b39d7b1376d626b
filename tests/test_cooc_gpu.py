"""GPU tests of the item-kNN from co-occurrence (anirec_cooc_scores, anirec_rows_topk, anirec_rows_rank,
anirec_itemknn_scores; ops / recs wrappers; the also_liked component and evaluate --baseline itemknn).

Yardstick: the NumPy restatement (tests/cooc_restatement.py).  Every comparison is exact, on bits, NaNs included; there
is no tolerance anywhere: counts are integers, the similarity is a fixed chain of correctly rounded fp64 operations, the
history scores are int64 sums of fixed-point terms.

Shapes: the smallest at which a kernel can go wrong — user counts around the 32-bit word, around the words a workgroup
stages per pass (anirec_cooc_chunk_words) and past two passes with a tail; item counts around the 64 x 64 tile; the
select at k on both sides of ANIREC_MAX_TOPK, with and without slices; the history scores on both sides of the LDS /
global switch (anirec_itemknn_lds_items)."""
import ctypes
import json
import os

import numpy as np
import pandas as pd
import pytest

import cooc_restatement as R
import poison
import recs_fixture as RF
from test_cooc_cpu import host_ops  # noqa: F401  (ops as the restatement, for the expected frames)
from test_recs_fixtures_gpu import _run

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
N_ITEMS = (1, 63, 64, 65, 130)
COMBOS = [(m, s, ms) for m in (R.COSINE, R.JACCARD, R.CONFIDENCE) for s in (0.0, 10.5) for ms in (0, 1, 3)]
NAMES = {v: k for k, v in R.MEASURES.items()}


def _cuda(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _u32(x):
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    return np.ascontiguousarray(a).view(np.uint32)


def _chunk():
    from anime_recommendations_amd import _lib
    return int(_lib.load().anirec_cooc_chunk_words())


def _n_users_cases():
    return (1, 31, 32, 33, 70, "32c-1", "32c+1", "64c+5")


def _n_users(case):
    c = _chunk()
    return {"32c-1": 32 * c - 1, "32c+1": 32 * c + 1, "64c+5": 64 * c + 5}.get(case, case)


def _liked(n_items, n_users, density, seed):
    rng = np.random.default_rng(seed)
    M = rng.random((n_items, n_users)) < density
    if n_items >= 3:
        M[0] = False                                            # an item nobody liked
        M[-1] = M[-2]                                           # twins
    return M


def _dirty_bits(M, seed):
    """the packed rows with garbage in the bits at positions >= n_users of every row's last word"""
    bits = R.pack_bits(M)
    tail = M.shape[1] % 32
    if tail:
        rng = np.random.default_rng(seed)
        bits[:, -1] |= (rng.integers(0, 1 << 32, len(bits), dtype=np.uint64).astype(np.uint32)
                        & np.uint32((0xFFFFFFFF << tail) & 0xFFFFFFFF))
    return bits


def _same_cooc(got, ref, what):
    sim, cnt, ex, pop = got
    rsim, rcnt, rex, rpop = ref
    assert np.array_equal(cnt.cpu().numpy(), rcnt), what
    assert np.array_equal(_u32(sim), _u32(rsim)), what
    assert np.array_equal(_u32(ex), rex), what
    assert np.array_equal(pop.cpu().numpy(), rpop), what


# ---- cooc_scores ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", N_ITEMS)
@pytest.mark.parametrize("users_case", _n_users_cases())
def test_cooc_scores_equals_the_restatement(users_case, n_items):
    from anime_recommendations_amd import ops
    n_users = _n_users(users_case)
    rng = np.random.default_rng(n_users * 131 + n_items)
    for density in (0.5, 0.02):
        M = _liked(n_items, n_users, density, n_users + n_items)
        clean, dirty = R.pack_bits(M), _dirty_bits(M, 7)
        bits = _cuda(dirty.view(np.int32))
        queries = np.concatenate([rng.permutation(n_items), [n_items - 1, 0, n_items, -1, n_items // 2]])
        for measure, shrink, min_support in COMBOS:
            what = (users_case, n_items, density, measure, shrink, min_support)
            sim, cnt, ex, pop, err = ops.cooc_scores(bits, n_users, queries, NAMES[measure], shrink, min_support, count=True,
                                                     excl=True, pop=True, check=False)
            ref = R.cooc_scores(clean, n_users, queries, measure, shrink, min_support)
            assert int(err.item()) == 1 == ref[4], what
            _same_cooc((sim, cnt, ex, pop), ref[:4], what)
        if n_items >= 3 and density == 0.5 and n_users >= 31:   # twins: exactly 1.0f at shrink 0
            sim = ops.cooc_scores(bits, n_users, [n_items - 1], "cosine", 0.0, 1)[0]
            assert float(sim[0, n_items - 2]) == 1.0 and float(sim[0, n_items - 1]) == 1.0 and float(sim[0, 0]) == 0.0
        with pytest.raises(ValueError, match="out of range"):
            ops.cooc_scores(bits, n_users, [0, n_items])
        only = ops.cooc_scores(bits, n_users, np.arange(n_items), count=True, excl=True, pop=True)     # no bad query: no flag
        _same_cooc(only, R.cooc_scores(clean, n_users, np.arange(n_items))[:4], "valid queries")


def test_a_query_alone_equals_its_row_in_a_batch_of_130():
    from anime_recommendations_amd import ops
    n_users = _n_users("64c+5")
    M = _liked(130, n_users, 0.3, 11)
    bits = _cuda(_dirty_bits(M, 3).view(np.int32))
    queries = np.random.default_rng(4).permutation(130)
    for measure in ("cosine", "jaccard", "confidence"):
        batch = ops.cooc_scores(bits, n_users, queries, measure, 10.5, 3, count=True, excl=True)
        for t in (0, 63, 64, 65, 129):
            one = ops.cooc_scores(bits, n_users, [int(queries[t])], measure, 10.5, 3, count=True, excl=True)
            for a, b in zip(one[:3], batch[:3]):
                assert np.array_equal(_u32(a[0]), _u32(b[t])), (measure, t)
        optional = ops.cooc_scores(bits, n_users, queries, measure, 10.5, 3)      # the optional outputs change nothing
        assert optional[1:] == (None, None, None) and np.array_equal(_u32(optional[0]), _u32(batch[0]))


@pytest.mark.parametrize("byte", poison.ORDER)
def test_cooc_scores_ignores_what_its_buffers_held(byte):
    from anime_recommendations_amd import ops
    n_users = _n_users("32c+1")
    M = _liked(65, n_users, 0.5, 5)
    bits = _cuda(_dirty_bits(M, 9).view(np.int32))
    queries = [3, 64, 0, 17]
    log = []
    with poison.poisoned(byte, log):
        got = ops.cooc_scores(bits, n_users, queries, "jaccard", 10.5, 3, count=True, excl=True, pop=True)
    assert len(log) >= 5
    _same_cooc(got, R.cooc_scores(R.pack_bits(M), n_users, queries, R.JACCARD, 10.5, 3)[:4], byte)


# ---- rows_topk --------------------------------------------------------------------------------------------------------
def _tables(n=300, n_users=40, dim=128, seed=0):
    rng = np.random.default_rng(seed)
    U = rng.normal(size=(n_users, dim)).astype(np.float32)
    A = rng.normal(size=(n, dim)).astype(np.float32)
    A[7] = A[3]                                                 # tied scores
    head = dict(w=1.3, b=-0.1, gamma=0.9, beta=0.05, mov_mean=0.02, mov_var=0.8)
    return _cuda(U), _cuda(A), head


@pytest.mark.parametrize("k", (1, 10, 128, 129, 300, 305))
def test_rows_topk_equals_the_lists_of_the_calls_that_made_the_rows(k):
    import torch
    from anime_recommendations_amd import ops
    U, A, head = _tables()
    n = 300
    Wh = ops.rownorm(A)
    queries = [5, 3, 7, 299, 0, 3]
    rows = torch.stack([ops.cosine_scores(Wh, q) for q in queries])
    keep = (np.arange(n) % 5 != 1).astype(np.uint8)
    want_i, want_s = ops.cosine_topk(Wh, queries, k, exclude_self=True, keep=keep)
    got_i, got_s = ops.rows_topk(rows, k, self_idx=queries, keep=keep)
    assert np.array_equal(got_i.cpu().numpy(), want_i.cpu().numpy()) and np.array_equal(_u32(got_s), _u32(want_s))
    users = np.arange(0, 40, 3)
    watched = np.random.default_rng(1).random((len(users), n)) < 0.3
    wb = _cuda(R.pack_bits(watched).view(np.int32))
    P = ops.predict_grid(U, A, head, users)
    want_i, want_s = ops.predict_topk(U, A, head, users, k, watched_bits=wb)
    got_i, got_s = ops.rows_topk(P, k, wbits=wb)
    assert np.array_equal(got_i.cpu().numpy(), want_i.cpu().numpy()) and np.array_equal(_u32(got_s), _u32(want_s))


def _special_rows(nq, n, ld, seed):
    rng = np.random.default_rng(seed)
    S = rng.integers(-3, 4, (nq, ld)).astype(np.float32) / 2     # many ties
    S[0, :] = np.nan
    S[1, ::3] = np.nan
    S[2, :] = 0.0
    S[2, ::2] = -0.0
    S[3, :] = 1.0
    S[:, n:] = 1e30                                             # past n: must never be listed
    return S


@pytest.mark.parametrize("n,ld,nq", [(300, 300, 7), (300, 317, 7), (5000, 5003, 5), (1, 4, 4), (33, 33, 1100)])
def test_rows_topk_order_masks_and_padding(n, ld, nq):
    from anime_recommendations_amd import ops
    S = _special_rows(max(nq, 4), n, ld, n + ld)[:nq]
    rng = np.random.default_rng(n)
    self_idx = rng.integers(-1, n, nq)
    keep = (rng.random(n) < 0.8).astype(np.uint8)
    W = rng.random((nq, n)) < 0.3
    wb = R.pack_bits(W)
    if n % 32:
        wb[:, -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)    # bits past n have no effect
    dS, dW = _cuda(S), _cuda(wb.view(np.int32))
    for k in sorted({1, 10, min(n, 128), n, n + 5}):
        for masks in (dict(), dict(self_idx=self_idx), dict(keep=keep), dict(wbits=dW),
                      dict(self_idx=self_idx, keep=keep, wbits=dW)):
            ref = dict(masks)
            if "wbits" in ref:
                ref["wbits"] = R.pack_bits(W)
            want_i, want_s = R.rows_topk(S, k, n, **ref)
            got_i, got_s = ops.rows_topk(dS, k, n, **masks)
            assert np.array_equal(got_i.cpu().numpy(), want_i), (k, list(masks))
            assert np.array_equal(_u32(got_s), _u32(want_s)), (k, list(masks))


@pytest.mark.parametrize("k", (10, 200))
def test_rows_topk_in_a_workspace_of_one_querys_share(k):
    import torch
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    n, nq = 300, 7
    S = _special_rows(nq, n, n, 3)
    dS = _cuda(S)
    want = ops.rows_topk(dS, k)
    one = int(lib.anirec_rows_topk_workspace_bytes(n, 1, k))
    assert one <= int(lib.anirec_rows_topk_workspace_bytes(n, nq, k))
    for byte in (0x00, 0xFF):
        ws = poison.fill(torch.empty(one, dtype=torch.uint8, device="cuda"), byte)
        got = ops.rows_topk(dS, k, workspace=ws)
        assert np.array_equal(got[0].cpu().numpy(), want[0].cpu().numpy()) and np.array_equal(_u32(got[1]), _u32(want[1]))
    assert np.array_equal(want[0].cpu().numpy(), R.rows_topk(S, k)[0])
    small = torch.empty(one - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.AnirecError, match="workspace"):
        ops.rows_topk(dS, k, workspace=small)


# ---- rows_rank --------------------------------------------------------------------------------------------------------
def test_rows_rank_with_ld_zero_is_score_rank():
    import torch
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(2)
    n, n_users, n_t = 333, 9, 500
    score = rng.integers(0, 20, n).astype(np.float32)
    score[5] = np.nan
    W = rng.random((n_users, n)) < 0.4
    tr, ta = rng.integers(0, n_users, n_t), rng.integers(0, n, n_t)
    ds, dw, dtr, dta = _cuda(score), _cuda(R.pack_bits(W).view(np.int32)), _cuda(tr.astype(np.int32)), _cuda(ta.astype(np.int32))
    want = ops.score_rank(ds, n_users, tr, ta, watched_bits=dw)
    rank = poison.fill(torch.empty(n_t, dtype=torch.int32, device="cuda"), 0x7F)
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x7F)
    st = lib.anirec_rows_rank(_lib.ptr(ds), 0, n, _lib.ptr(dw), n_users, _lib.ptr(dtr), _lib.ptr(dta), n_t, _lib.ptr(rank),
                              _lib.ptr(err), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0 and int(err.item()) == 0
    assert np.array_equal(rank.cpu().numpy(), want.cpu().numpy())
    assert np.array_equal(rank.cpu().numpy(), R.rows_rank(score, 0, n, R.pack_bits(W), n_users, tr, ta)[0])


def test_rows_rank_is_the_position_in_rows_topk():
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(3)
    n, n_users = 131, 6
    S = _special_rows(n_users, n, n, 8)
    W = rng.random((n_users, n)) < 0.3
    tr, ta = np.repeat(np.arange(n_users), 20), rng.integers(0, n, n_users * 20)
    dS = _cuda(S)
    rank = ops.rows_rank(dS, tr, ta, watched_bits=_cuda(R.pack_bits(W).view(np.int32))).cpu().numpy()
    assert np.array_equal(rank, R.rows_rank(S, n, n, R.pack_bits(W), n_users, tr, ta)[0])
    for t in range(len(tr)):
        w = W[tr[t]].copy()
        w[ta[t]] = False                                        # the target's own bit cleared
        idx, _ = ops.rows_topk(dS[tr[t]:tr[t] + 1], n, wbits=_cuda(R.pack_bits(w[None]).view(np.int32)))
        assert int(idx[0, rank[t]]) == ta[t], t
    for bad_r, bad_a in ((n_users, 0), (-1, 0), (0, n), (0, -1)):
        with pytest.raises(ValueError, match="out of range"):
            ops.rows_rank(dS, [0, bad_r], [1, bad_a])


# ---- itemknn_scores ---------------------------------------------------------------------------------------------------
def _knn_case(n, K, n_lists, seed, max_len=9):
    rng = np.random.default_rng(seed)
    ni = rng.integers(-1, n, (n, K)).astype(np.int32)           # -1 padding among them
    ns = rng.random((n, K)).astype(np.float32)
    ns[rng.random((n, K)) < 0.1] *= -1
    lens = rng.integers(0, max_len + 1, n_lists)
    lens[1 % n_lists] = 0                                       # an empty history
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    hi = rng.integers(0, n, int(off[-1])).astype(np.int32)
    if lens[0] >= 2:
        hi[1] = hi[0]                                           # a repeated item
    hw = (rng.random(len(hi)) * 4).astype(np.float32)
    return ni, ns, off, hi, hw


def _lds_items():
    from anime_recommendations_amd import _lib
    return int(_lib.load().anirec_itemknn_lds_items())


@pytest.mark.parametrize("n_case", (1, 50, 777, "lds", "lds+1"))
def test_itemknn_scores_equals_the_restatement(n_case):
    from anime_recommendations_amd import ops
    n = {"lds": _lds_items(), "lds+1": _lds_items() + 1}.get(n_case, n_case)
    K, n_lists = (3, 4) if n > 1000 else (5, 9)
    ni, ns, off, hi, hw = _knn_case(n, K, n_lists, n)
    dni, dns = _cuda(ni), _cuda(ns)
    for w in (hw, None):
        want, err = R.itemknn_scores(ni, ns, off, hi, w)
        assert err == 0
        got = ops.itemknn_scores(dni, dns, off, hi, w)
        assert np.array_equal(_u32(got), _u32(want)), n_case
        assert not got[1 % n_lists].any() and not np.signbit(got[1 % n_lists].cpu().numpy()).any()     # empty history: +0
    ones = ops.itemknn_scores(dni, dns, off, hi, np.ones(len(hi), np.float32))
    assert np.array_equal(_u32(ones), _u32(ops.itemknn_scores(dni, dns, off, hi, None)))
    # permuted histories, a list alone, a poisoned workspace: the same bits
    rng = np.random.default_rng(1)
    hi2, hw2 = hi.copy(), hw.copy()
    for l in range(n_lists):
        p = rng.permutation(off[l + 1] - off[l]) + off[l]
        hi2[off[l]:off[l + 1]], hw2[off[l]:off[l + 1]] = hi[p], hw[p]
    full = ops.itemknn_scores(dni, dns, off, hi, hw)
    assert np.array_equal(_u32(ops.itemknn_scores(dni, dns, off, hi2, hw2)), _u32(full))
    for l in (0, n_lists - 1):
        alone = ops.itemknn_scores(dni, dns, off[l:l + 2], hi, hw)
        assert np.array_equal(_u32(alone[0]), _u32(full[l])), l
    for byte in (0x3F, 0xFF):
        with poison.poisoned(byte, []):
            again = ops.itemknn_scores(dni, dns, off, hi, hw)
        assert np.array_equal(_u32(again), _u32(full)), byte


@pytest.mark.parametrize("n_case", (50, "lds+1"))
def test_itemknn_scores_flags_bad_values_and_isolates_them(n_case):
    from anime_recommendations_amd import ops
    n = {"lds+1": _lds_items() + 1}.get(n_case, n_case)
    K, n_lists = 3, 4
    ni, ns, off, hi, hw = _knn_case(n, K, n_lists, 5, max_len=6)
    off = np.array([0, 3, 3, 6, 9], np.int32)
    hi, hw = (np.arange(9) * 7 % n).astype(np.int32), (np.arange(9) % 4 + 0.5).astype(np.float32)
    for what in ("item", "item-", "neighbour", "offsets", "past", "nan", "inf", "large"):
        ni2, ns2, off2, hi2, hw2 = ni.copy(), ns.copy(), off.copy(), hi.copy(), hw.copy()
        if what == "item":
            hi2[7] = n
        elif what == "item-":
            hi2[7] = -1
        elif what == "neighbour":
            ni2[hi[7], 1] = n
        elif what == "offsets":
            off2[3] = 2                                         # lists 2 and 3 are (3, 2) and (2, 9)
        elif what == "past":
            off2[4] = 10                                        # past the history
        elif what == "nan":
            hw2[7] = np.nan
        elif what == "inf":
            ns2[hi[7], 0], ni2[hi[7], 0] = np.inf, 1 % n
        else:
            hw2[7], ns2[hi[7], 0], ni2[hi[7], 0] = 2000.0, 0.75, 1 % n
        want, err = R.itemknn_scores(ni2, ns2, off2, hi2, hw2)
        assert err == 1, what
        got, flag = ops.itemknn_scores(_cuda(ni2), _cuda(ns2), off2, hi2, hw2, check=False)
        assert int(flag.item()) == 1, what
        assert np.array_equal(_u32(got), _u32(want)), what
        with pytest.raises(ValueError, match="out of range"):
            ops.itemknn_scores(_cuda(ni2), _cuda(ns2), off2, hi2, hw2)


# ---- graph capture ----------------------------------------------------------------------------------------------------
def test_scores_and_select_replay_from_a_graph():
    """(a) + (b) captured into one graph run nothing; each replay writes the restatement's bits"""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    n_items, n_users, k = 130, _n_users("32c+1"), 10
    M = _liked(n_items, n_users, 0.3, 21)
    bits = _cuda(_dirty_bits(M, 2).view(np.int32))
    queries = _cuda(np.arange(n_items, dtype=np.int32))
    ew = (n_items + 31) // 32
    shapes = ((n_items * n_items, torch.float32), (n_items * n_items, torch.int32), (n_items * ew, torch.int32),
              (n_items, torch.int32), (1, torch.int32), (n_items * k, torch.int32), (n_items * k, torch.float32))
    sim, cnt, ex, pop, err, idx, val = [poison.fill(torch.empty(m, dtype=dt, device="cuda"), 0x3F) for m, dt in shapes]
    ws_a = poison.fill(torch.empty(int(lib.anirec_cooc_workspace_bytes(n_items, n_items)), dtype=torch.uint8, device="cuda"), 0x3F)
    ws_b = poison.fill(torch.empty(int(lib.anirec_rows_topk_workspace_bytes(n_items, n_items, k)), dtype=torch.uint8,
                                   device="cuda"), 0x3F)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st_a = lib.anirec_cooc_scores(_lib.ptr(bits), n_items, n_users, _lib.ptr(queries), n_items, R.COSINE, 10.5, 2,
                                      _lib.ptr(sim), _lib.ptr(cnt), _lib.ptr(ex), _lib.ptr(pop), _lib.ptr(err), _lib.ptr(ws_a),
                                      ws_a.numel(), s)
        st_b = lib.anirec_rows_topk(_lib.ptr(sim), n_items, n_items, n_items, None, None, _lib.ptr(ex), k, _lib.ptr(idx),
                                    _lib.ptr(val), _lib.ptr(ws_b), ws_b.numel(), s)
    assert st_a == 0 and st_b == 0
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0x3F).all()) for t in (sim, cnt, ex, pop, err, idx, val))   # captured, not run
    rsim, rcnt, rex, rpop, _ = R.cooc_scores(R.pack_bits(M), n_users, np.arange(n_items), R.COSINE, 10.5, 2)
    ri, rv = R.rows_topk(rsim, k, wbits=rex)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        _same_cooc((sim.view(n_items, n_items), cnt.view(n_items, n_items), ex.view(n_items, ew), pop), (rsim, rcnt, rex, rpop),
                   "replay")
        assert np.array_equal(idx.view(n_items, k).cpu().numpy(), ri) and np.array_equal(_u32(val.view(n_items, k)), _u32(rv))
        for t in (idx, val):
            poison.fill(t, 0x7F)


# ---- a planted set ----------------------------------------------------------------------------------------------------
def _planted():
    """two disjoint communities: users 0 .. 19 like items 0 .. 9, users 20 .. 59 items 10 .. 21 (user u likes item i of
    its community unless (u + i) % 3 == 0); every user of the SMALLER community has one liked item held out"""
    nA, nB, iA, iB = 20, 40, 10, 12
    L = np.zeros((nA + nB, iA + iB), bool)
    for u in range(nA + nB):
        items = range(iA) if u < nA else range(iA, iA + iB)
        for i in items:
            L[u, i] = (u + i) % 3 != 0
    held = np.array([[u, np.flatnonzero(L[u])[u % int(L[u].sum())]] for u in range(nA)])
    train = L.copy()
    train[held[:, 0], held[:, 1]] = False
    assert train.sum(axis=0).min() >= 5
    return train, held, iA, iB


def _planted_ranks(cooc, topk, knn_scores, rank, score_rank):
    train, held, iA, iB = _planted()
    n_users, n_items = train.shape
    bits = R.pack_bits(train.T)
    sim, _, excl, pop = cooc(bits, n_users, np.arange(n_items))
    ni, ns = topk(sim, iA - 1, excl)
    users = held[:, 0]
    off = np.concatenate([[0], np.cumsum(train[users].sum(axis=1))]).astype(np.int32)
    hist = np.concatenate([np.flatnonzero(train[u]) for u in users]).astype(np.int32)
    scores = knn_scores(ni, ns, off, hist)
    seen = R.pack_bits(train[users])
    knn_rank = rank(scores, np.arange(len(users)), held[:, 1], seen)
    pop_rank = score_rank(pop.astype(np.float32), len(users), np.arange(len(users)), held[:, 1], seen)
    return ni, knn_rank, pop_rank, iA, iB


def _check_planted(ni, knn_rank, pop_rank, iA, iB):
    for i in range(iA + iB):                                    # every neighbour is of the item's own community
        own = ni[i][ni[i] >= 0]
        assert len(own) >= 5 and ((own < iA) == (i < iA)).all(), i
    assert (knn_rank >= 0).all() and (knn_rank < pop_rank).all()
    assert (knn_rank < iA).all() and (pop_rank >= iB).all()     # why: the larger community's items are the popular ones


def test_planted_communities_on_the_restatement():
    _check_planted(*_planted_ranks(
        lambda b, nu, q: [R.cooc_scores(b, nu, q)[i] for i in (0, 1, 2, 3)],
        lambda s, k, ex: R.rows_topk(s, k, wbits=ex),
        lambda ni, ns, off, h: R.itemknn_scores(ni, ns, off, h)[0],
        lambda sc, tr, ta, seen: R.rows_rank(sc, sc.shape[1], sc.shape[1], seen, sc.shape[0], tr, ta)[0],
        lambda p, nu, tr, ta, seen: R.rows_rank(p, 0, len(p), seen, nu, tr, ta)[0]))


def test_planted_communities_on_the_gpu():
    from anime_recommendations_amd import ops
    i32 = lambda b: _cuda(np.ascontiguousarray(b).view(np.int32))
    got = _planted_ranks(
        lambda b, nu, q: [x.cpu().numpy() for x in ops.cooc_scores(i32(b), nu, q, count=True, excl=True, pop=True)],
        lambda s, k, ex: [x.cpu().numpy() for x in ops.rows_topk(_cuda(s), k, wbits=i32(ex))],
        lambda ni, ns, off, h: ops.itemknn_scores(_cuda(ni), _cuda(ns), off, h).cpu().numpy(),
        lambda sc, tr, ta, seen: ops.rows_rank(_cuda(sc), tr, ta, watched_bits=i32(seen)).cpu().numpy(),
        lambda p, nu, tr, ta, seen: ops.score_rank(_cuda(p), nu, tr, ta, watched_bits=i32(seen)).cpu().numpy())
    _check_planted(*got)
    want = _planted_ranks(
        lambda b, nu, q: [R.cooc_scores(b, nu, q)[i] for i in (0, 1, 2, 3)],
        lambda s, k, ex: R.rows_topk(s, k, wbits=ex),
        lambda ni, ns, off, h: R.itemknn_scores(ni, ns, off, h)[0],
        lambda sc, tr, ta, seen: R.rows_rank(sc, sc.shape[1], sc.shape[1], seen, sc.shape[0], tr, ta)[0],
        lambda p, nu, tr, ta, seen: R.rows_rank(p, 0, len(p), seen, nu, tr, ta)[0])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    # the recs layer on the same set: fit, lists and ranks in batches of 7 users / 5 items
    from anime_recommendations_amd import recs
    train, held, iA, iB = _planted()
    u, a = np.nonzero(train)
    knn = recs.itemknn_fit(u, a, np.ones(len(u)), train.shape[0], train.shape[1], 0.5, iA - 1)
    assert np.array_equal(knn["nbr_idx"].cpu().numpy(), want[0]) and knn["pop"].cpu().numpy().tolist() == train.sum(axis=0).tolist()
    idx, sim, cnt = recs.cooc_neighbours(i32(R.pack_bits(train.T)), train.shape[0], iA - 1, batch=5)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(_u32(sim), _u32(knn["nbr_sim"]))
    both = (train.T.astype(np.int64) @ train.astype(np.int64))
    ok = want[0] >= 0
    assert np.array_equal(cnt.cpu().numpy()[ok], both[np.nonzero(ok)[0], want[0][ok]]) and (cnt.cpu().numpy()[~ok] == -1).all()
    off, hist, _ = recs.history_csr(u, a, np.ones(len(u), np.float32), held[:, 0])
    seen = i32(R.pack_bits(train[held[:, 0]]))
    r = recs.itemknn_rank(knn, off, hist, None, seen, np.arange(len(held)), held[:, 1], batch=7)
    assert np.array_equal(r.cpu().numpy(), want[1])
    li, ls = recs.itemknn_topk(knn, off, hist, None, 3, seen, batch=7)
    assert (li.cpu().numpy() < iA).all() and (np.diff(ls.cpu().numpy(), axis=1) <= 0).all()
    rr = r.cpu().numpy()
    assert all(int(li[t, rr[t]]) == held[t, 1] for t in range(len(held)) if rr[t] < 3)


# ---- the components, end to end on the recs fixture -------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_store(tmp_path_factory):
    from anime_recommendations_amd import artifacts, components as C, weights_io
    work = tmp_path_factory.mktemp("cooc")
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(work / "store"))
    old = os.environ.get("ANIREC_ARTIFACT_DIR")
    os.environ["ANIREC_ARTIFACT_DIR"] = env["ANIREC_ARTIFACT_DIR"]
    rec = RF.load()
    z, df = rec["npz"], RF.ratings(rec)
    user_ids, anime_ids = C.index_tables({}, df)
    pq = str(work / "user_stats.parquet")
    df.to_parquet(pq, index=False)
    (work / "all_anime.csv").write_bytes(z["anime_csv"].tobytes())
    (work / "synopses.csv").write_bytes(z["synopses_csv"].tobytes())
    mp = str(work / "wandb_anime_nn.h5")
    weights_io.save_model(mp, z["U"], z["A"], dict(rec["model_recs"]["heads"]["sigmoid"], activation="sigmoid"),
                          user_ids=user_ids, anime_ids=anime_ids)
    for name, path, kind in (("user_stats.parquet", pq, "parquet"), ("all_anime.csv", str(work / "all_anime.csv"), "raw_data"),
                             ("synopses.csv", str(work / "synopses.csv"), "raw_data"), ("wandb_anime_nn.h5", mp, "h5")):
        artifacts.log_artifact(name, path, kind)
    yield dict(work=work, env=env, rec=rec, df=df, pq=pq)
    if old is None:
        os.environ.pop("ANIREC_ARTIFACT_DIR", None)
    else:
        os.environ["ANIREC_ARTIFACT_DIR"] = old


def test_also_liked_component_on_the_recs_fixture(fixture_store, request):
    from anime_recommendations_amd import artifacts, components as C
    work, env, rec, df = (fixture_store[k] for k in ("work", "env", "rec", "df"))
    flags, query = rec["flags"], rec["similar_anime"]["cases"][0]["query"]
    al = dict(project_name="anime_recommendations", main_df="user_stats.parquet:latest", main_df_type="parquet",
              anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopses_df="synopses.csv:latest",
              sypnopsis_df_type="raw_data", anime_query=query, a_query_number=25, random_anime=False,
              anime_rec_genres=flags["SA_GENRES"], an_spec_genres=False, types=flags["SA_TYPES"], spec_types=True,
              a_rec_type="csv", save_sim_anime=True, liked_min_rating=0.6, cooc_measure="jaccard", cooc_shrink=10.5,
              cooc_min_support=2)
    _run("also_liked", al, str(work), env)
    fn = C.clean(query) + "_also_liked.csv"
    got = (work / fn).read_text()
    meta = artifacts.artifact_metadata(fn + ":latest")
    assert meta["cooc_measure"] == "jaccard" and meta["cooc_min_support"] == 2 and meta["Queried anime"] == query
    anime_df = C.load_anime_df(RF.csv(rec, "anime_csv"))
    syn_df = C.load_synopses(RF.csv(rec, "synopses_csv"))
    gpu_frame, _ = C.also_liked_frame(df, anime_df, syn_df, query, 25, types=C.literal(flags["SA_TYPES"]),
                                      liked_min_rating=0.6, measure="jaccard", shrink=10.5, min_support=2)
    assert got == gpu_frame.to_csv(index=False)
    request.getfixturevalue("host_ops")                          # from here on ops is the restatement
    want, want_fn = C.also_liked_frame(df, anime_df, syn_df, query, 25, types=C.literal(flags["SA_TYPES"]),
                                       liked_min_rating=0.6, measure="jaccard", shrink=10.5, min_support=2)
    assert want_fn == fn and got == want.to_csv(index=False)
    assert 0 < len(want) <= 25 and (want["Liked_by_both"] >= 2).all() and (np.diff(want["Similarity"]) <= 0).all()
    assert want["Type"].isin(C.literal(flags["SA_TYPES"])).all() and query not in want["Name"].tolist()


def test_evaluate_baseline_itemknn_on_the_recs_fixture(fixture_store):
    from anime_recommendations_amd import data, recs
    work, env, pq = fixture_store["work"], fixture_store["env"], fixture_store["pq"]
    ks = [1, 5, 20]
    ev = dict(input_data="user_stats.parquet:latest", main_df_type="parquet", model="wandb_anime_nn.h5:latest",
              model_type="h5", project_name="anime_recommendations", test_size=1000, eval_k=str(ks), min_rating=0.7,
              eval_csv="ranking_metrics.csv", eval_type="eval_csv", ID_emb_name="user_embedding",
              anime_emb_name="anime_embedding")
    from anime_recommendations_amd import artifacts, components as C, weights_io
    from test_rank_gpu import _run as _run_out
    code, out = _run_out("evaluate", dict(ev, baseline="popularity,itemknn", itemknn_neighbours=20, itemknn_measure="jaccard",
                                          itemknn_shrink=10.5, itemknn_min_support=2, itemknn_min_rating=0.6), str(work), env)
    assert code == 0, out[-3000:]
    summary = json.loads(out.strip().splitlines()[-1])
    frame = pd.read_csv(work / "ranking_metrics.csv", float_precision="round_trip")
    assert frame.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity", "hit_rate_itemknn",
                                      "ndcg_itemknn"]
    # the model's and the popularity columns are what the frame function gives without the item-kNN, to the byte
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    plain_frame, plain = C.evaluate_frame(model, data.load_user_stats(pq), 1000, ks, 0.7)
    pop_frame, pop = C.evaluate_frame(model, data.load_user_stats(pq), 1000, ks, 0.7, baseline="popularity")
    assert frame[["k", "hit_rate", "ndcg"]].to_csv(index=False) == plain_frame.to_csv(index=False)
    assert frame[frame.columns[:5]].to_csv(index=False) == pop_frame.to_csv(index=False)
    assert {k: summary[k] for k in plain} == plain and {k: summary[k] for k in pop} == pop
    assert list(summary)[:len(pop)] == list(pop) and list(pop)[:len(plain)] == list(plain)
    # the item-kNN figures from the restatement alone, fitted on the training slice
    table = data.load_user_stats(pq)
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    assert len(row) > 100
    tu, ta, tr = table.user[train], table.anime[train], table.rating[train].astype(np.float32)
    liked = tr >= np.float32(0.6)
    L = np.zeros((table.n_anime, table.n_users), bool)
    L[ta[liked], tu[liked]] = True
    sim, _, excl, _, _ = R.cooc_scores(R.pack_bits(L), table.n_users, np.arange(table.n_anime), R.JACCARD, 10.5, 2)
    ni, ns = R.rows_topk(sim, 20, wbits=excl)
    off = np.concatenate([[0], np.cumsum([int(((tu == u) & liked).sum()) for u in users])])
    hist = np.concatenate([ta[(tu == u) & liked] for u in users])
    scores, err = R.itemknn_scores(ni, ns, off, hist)
    seen = np.zeros((len(users), table.n_anime), bool)
    for i, u in enumerate(users):
        seen[i, ta[tu == u]] = True
    rank, err2 = R.rows_rank(scores, table.n_anime, table.n_anime, R.pack_bits(seen), len(users), row, anime)
    assert err == 0 and err2 == 0
    b = recs.ranking_metrics(rank, ks)
    assert frame["hit_rate_itemknn"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_itemknn"].tolist() == [b["ndcg"][k] for k in ks]
    assert summary["itemknn_mrr"] == b["mrr"] and summary["itemknn_mean_rank"] == b["mean_rank"]
