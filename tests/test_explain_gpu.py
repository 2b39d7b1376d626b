"""GPU tests of the explained lists (anirec_explain_lists, ops.explain_lists, recs.explain_topk,
components.explain_recs_frame, the explain_recs component).

Yardstick: the NumPy restatement (tests/explain_restatement.py) run on the similarities the existing
``ops.cosine_scores`` returns for the same normalised table — that kernel is not under test here, and the header defines
sim(s, i) as its chain, bit for bit.  Every comparison of pos, sim and contrib is exact, on bits, NaNs included.

Shapes: test_mmr_gpu's 777-row tables (widths 32, 64, 128, 256, with two bit-identical rows and a zero row), 37 lists a
call; k 1, 2, 10, 33 and anirec_explain_max_k(width); m 1, 3, 8; history lengths 0, 1, m - 1, m, m + 1 and T - 1, T,
T + 1, 3 T + 5 around the tile T = anirec_explain_tile(width, k) the kernel stages per pass.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest

import explain_restatement as E
import poison
from test_components_gpu import _run, pipeline  # noqa: F401  (the components' pipeline fixture, as it is)
from test_listeval_gpu import HEAD, _small_model
from test_mmr_gpu import N_LISTS, N_ROWS, TWIN_A, TWIN_B, WIDTHS, ZERO_ROW, _bits, _cuda, _table

pytestmark = pytest.mark.gpu
KS = (1, 2, 10, 33, "max")
MS = (1, 3, 8)
NAN_BITS = np.uint32(0x7FC00000)
BAD_LIST = 21


def _k(dim, k):
    from anime_recommendations_amd import _lib
    return _lib.explain_max_k(dim) if k == "max" else k


def _tile(dim, k):
    from anime_recommendations_amd import _lib
    return _lib.explain_tile(dim, k)


def _case(dim, k, m, seed=0):
    """(list_idx [N_LISTS, k], offsets, hist_idx, weight): random rows and ratings 0.1 .. 1.0, lists 0 .. 8 with the
    content that takes a path of its own, lists 10 .. 36 three rounds of the nine history lengths."""
    rng = np.random.default_rng(seed * 100000 + dim * 100 + k * 10 + m)
    T = _tile(dim, k)
    lengths = [0, 1, m - 1, m, m + 1, T - 1, T, T + 1, 3 * T + 5]
    idx = rng.integers(0, N_ROWS, (N_LISTS, k)).astype(np.int32)
    idx[idx == ZERO_ROW] = ZERO_ROW + 1
    mid = k // 2
    n = [lengths[(l - 10) % 9] for l in range(N_LISTS)]
    n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8], n[9] = T + 1, m + 1, T + 1, m + 4, m + 2, 4, T, T + 6, 3 * T + 5, T
    hist = [rng.integers(0, N_ROWS, x).astype(np.int32) for x in n]
    for h in hist:
        h[h == ZERO_ROW] = ZERO_ROW + 1
    w = [(rng.integers(1, 11, x) / 10.0).astype(np.float32) for x in n]
    idx[0, [0, mid, k - 1]] = -1                                # empty slots at the front, the middle and the end
    idx[1, :] = -1                                              # an all-empty list
    idx[2, 0] = ZERO_ROW                                        # the zero row (NaN once normalised) as a slot ...
    hist[3][1] = ZERO_ROW                                       # ... and as a history entry
    hist[4][2], w[4][2] = hist[4][0], w[4][0]                   # a repeated history anime with one weight: a tie
    hist[5][:] = [20, TWIN_B, 21, TWIN_A]                       # two bit-identical rows with equal weights, the rest tiny
    w[5][:] = [1e-3, 1.0, 1e-3, 1.0]
    hist[6][0], w[6][0] = idx[6, 0], 1.0                        # a history entry equal to a listed row
    w[7][:5] = [0.0, -0.0, -0.5, np.inf, np.nan]                # weights 0, -0, negative, inf and NaN
    w[8][:] = 0.0                                               # all weights zero: every contrib +-0, all tied
    offsets = np.zeros(N_LISTS + 1, np.int64)
    np.cumsum(n, out=offsets[1:])
    return idx, offsets, np.concatenate(hist), np.concatenate(w)


_REFS = {}


def _reference(dim, k, m, seed=0):
    key = (dim, k, m, seed)
    if key not in _REFS:
        _REFS[key] = E.explain_lists(_table(dim)[2], *_case(dim, k, m, seed), m)
    return _REFS[key]


def _same(got, ref, what):
    gp, gs, gc = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in got]
    assert np.array_equal(gp, ref[0]), what
    assert np.array_equal(_bits(gs), _bits(ref[1])), what
    assert np.array_equal(_bits(gc), _bits(ref[2])), what


def _run_case(dim, case, m):
    from anime_recommendations_amd import ops
    idx, off, hist, w = case
    return ops.explain_lists(_table(dim)[0], _cuda(idx), off, _cuda(hist), _cuda(w), m)


def _take(case, order):
    """the lists ``order`` of a case as a call of their own"""
    idx, off, hist, w = case
    n = off[1:] - off[:-1]
    new = np.zeros(len(order) + 1, np.int64)
    np.cumsum(n[order], out=new[1:])
    pick = np.concatenate([np.arange(off[l], off[l + 1]) for l in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    return idx[order], new, hist[pick], w[pick]


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_explain_equals_the_restatement(dim, k, m):
    k = _k(dim, k)
    case = _case(dim, k, m)
    ref = _reference(dim, k, m)
    _same(_run_case(dim, case, m), ref, (dim, k, m))
    _check_plants(dim, k, m, case, ref, _table(dim)[2])


def _check_plants(dim, k, m, case, ref, S):
    """the planted content did what it is there for (checked on the reference, which the kernel has just equalled)"""
    T = _tile(dim, k)
    idx, off, hist, w = case
    rp, rs, rc = ref
    lens = set((off[1:] - off[:-1]).tolist())
    assert {0, 1, m - 1, m, m + 1, T - 1, T, T + 1, 3 * T + 5} <= lens
    assert (rp[0, [0, k // 2, k - 1]] == -1).all() and (_bits(rs[0, [0, k // 2, k - 1]]) == NAN_BITS).all()
    assert (rp[1] == -1).all() and (_bits(rs[1]) == NAN_BITS).all() and (_bits(rc[1]) == NAN_BITS).all()
    assert (rp[2, 0] == -1).all() and (_bits(rc[2, 0]) == NAN_BITS).all()       # a NaN slot picks nothing
    if k >= 2:
        assert (rp[2, 1] >= 0).all()                                             # ... and leaves its neighbours alone
    present3 = idx[3] >= 0
    assert (rp[3][present3] != 1).all() and (rp[3][present3][:, :min(m, 3)] >= 0).all()   # the NaN entry is never picked
    for s in range(k):                                           # the repeated anime: position 0 directly before 2
        at0 = np.flatnonzero(rp[4, s] == 0)
        if len(at0) and at0[0] + 1 < m:
            assert rp[4, s, at0[0] + 1] == 2 and _bits(rc[4, s, at0[0]]) == _bits(rc[4, s, at0[0] + 1])
    assert (rp[4, :, 0] != 2).all()
    assert _bits(S[idx[5, 0], TWIN_A]) == _bits(S[idx[5, 0], TWIN_B])
    for s in range(k):                                           # the twins: position 1 directly before position 3
        ranks = rp[5, s].tolist()
        assert 3 not in ranks or (1 in ranks and ranks.index(3) == ranks.index(1) + 1)
        assert m < 4 or (1 in ranks and 3 in ranks)
    r6 = np.flatnonzero(rp[6, 0] == 0)
    assert len(r6) == 1 and rs[6, 0, r6[0]] > 0.999                # the listed row itself, found in the history
    c7 = w[off[7]:off[7] + 5] * S[idx[7, 0], hist[off[7]:off[7] + 5]]
    assert np.isnan(c7[4]) and np.isinf(c7[3]) and c7[0] == 0 and c7[1] == 0 and np.signbit(w[off[7] + 1]) and c7[2] != 0
    if c7[3] > 0:                                                # +inf first, -inf after everything, the NaN weight nowhere
        assert rp[7, 0, 0] == 3 and rc[7, 0, 0] == np.inf
    else:
        assert (rp[7, 0] != 3).all()
    assert (rp[7] != 4).all()
    assert (rp[8] == np.arange(m)).all() and (rc[8] == 0).all()                  # all tied at +-0: positions 0 .. m - 1


def test_a_permuted_history_gives_the_same_picks():
    """the order is total wherever no two contribs tie, so the same history in another order — other lanes, other
    tiles — gives every slot the same (history row, contrib) sequence; weights from a continuous draw, the no-tie
    condition asserted on the similarities"""
    from anime_recommendations_amd import ops
    dim, k, m = 128, 10, 8
    Wh, _, S = _table(dim)
    T = _tile(dim, k)
    rng = np.random.default_rng(17)
    rows = np.setdiff1d(np.arange(N_ROWS), [ZERO_ROW, TWIN_B])
    idx = rng.choice(rows, (N_LISTS, k)).astype(np.int32)
    n = 3 * T + 5
    hist = np.stack([rng.permutation(rows)[:n] for _ in range(N_LISTS)]).astype(np.int32)
    w = rng.uniform(0.1, 1.0, (N_LISTS, n)).astype(np.float32)
    for l in range(N_LISTS):
        c = w[l][None, :] * S[np.ix_(idx[l], hist[l])]
        assert all(len(np.unique(row)) == n for row in c)       # no two contribs of a slot tie
    perm = np.stack([rng.permutation(n) for _ in range(N_LISTS)])
    hist2, w2 = np.take_along_axis(hist, perm, 1), np.take_along_axis(w, perm, 1)
    off = np.arange(N_LISTS + 1, dtype=np.int64) * n
    a = [t.cpu().numpy() for t in ops.explain_lists(Wh, _cuda(idx), off, _cuda(hist.reshape(-1)), _cuda(w.reshape(-1)), m)]
    b = [t.cpu().numpy() for t in ops.explain_lists(Wh, _cuda(idx), off, _cuda(hist2.reshape(-1)), _cuda(w2.reshape(-1)), m)]
    assert (a[0] >= 0).all() and (b[0] >= 0).all() and not np.array_equal(a[0], b[0])
    for l in range(N_LISTS):
        assert np.array_equal(hist[l][a[0][l]], hist2[l][b[0][l]]), l
    assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))


def test_a_list_does_not_depend_on_its_context():
    """a list run alone, at another position among other lists, and twice: the same bits — for a short list and for the
    longest one (lists 8, 18, 27 and 36 hold histories of 3 T + 5 entries)"""
    for dim, k, m in ((128, 10, 3), (128, "max", 8)):
        k = _k(dim, k)
        case = _case(dim, k, m)
        ref = _reference(dim, k, m)
        assert case[1][37] - case[1][36] > 3 * _tile(dim, k) and case[1][9] - case[1][8] > 3 * _tile(dim, k)
        _same(_run_case(dim, case, m), ref, "whole call")
        _same(_run_case(dim, case, m), ref, "second run")
        perm = np.random.default_rng(5).permutation(N_LISTS)
        _same(_run_case(dim, _take(case, perm), m), [r[perm] for r in ref], "permuted call")
        for l in (0, 7, 8, 17, 36):
            _same(_run_case(dim, _take(case, [l]), m), [r[l:l + 1] for r in ref], "list %d alone" % l)


@pytest.mark.parametrize("byte", poison.ORDER)
def test_dirty_outputs_are_fully_overwritten(byte):
    for dim, k, m in ((32, 33, 1), (128, 10, 3), (256, 64, 8)):
        case = _case(dim, k, m)
        log = []
        with poison.poisoned(byte, log):
            got = _run_case(dim, case, m)
        assert len(log) == 4 and sum(log) == N_LISTS * k * m * 12 + 4           # the three outputs and the flag word
        _same(got, _reference(dim, k, m), (byte, dim))


def _raw(dim, case, m, k=None, n_rows=N_ROWS, n_lists=None, null=None, fill=0x3F, dim_arg=None):
    """anirec_explain_lists itself, its outputs and flag pre-filled with ``fill`` bytes: no wrapper check between the test
    and the entry point.  ``null``: the name of one pointer passed as NULL.  Returns (status, outs, err)."""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    idx, off, hist, w = case
    k = idx.shape[1] if k is None else k
    shape = (idx.shape[0], max(k, idx.shape[1]), max(m, 1))
    outs = [poison.fill(torch.empty(shape, dtype=dt, device="cuda"), fill) for dt in (torch.int32, torch.float32, torch.float32)]
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), fill)
    p = dict(What=_table(dim)[0], list_idx=_cuda(idx), off=_cuda(off), hidx=_cuda(hist), hw=_cuda(w), pos=outs[0],
             sim=outs[1], contrib=outs[2], err=err)
    if null:
        p[null] = None
    st = lib.anirec_explain_lists(_lib.ptr(p["What"]), dim if dim_arg is None else dim_arg, n_rows, _lib.ptr(p["list_idx"]),
                                  idx.shape[0] if n_lists is None else n_lists, k, _lib.ptr(p["off"]), _lib.ptr(p["hidx"]),
                                  _lib.ptr(p["hw"]), m, _lib.ptr(p["pos"]), _lib.ptr(p["sim"]), _lib.ptr(p["contrib"]),
                                  _lib.ptr(p["err"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, outs, err


def _poisoned_ref(ref, l):
    ref = [r.copy() for r in ref]
    ref[0][l], ref[1][l], ref[2][l] = -1, np.nan, np.nan
    return ref


def _bad_value_round(dim, k, m, case, ref):
    from anime_recommendations_amd import ops
    st, outs, err = _raw(dim, case, m)
    assert st == 0 and int(err.item()) == 1
    _same(outs, ref, "bad value")
    with pytest.raises(ValueError, match="out of range|offsets"):
        ops.explain_lists(_table(dim)[0], _cuda(case[0]), case[1], _cuda(case[2]), _cuda(case[3]), m)
    st, outs, err = _raw(dim, _case(dim, k, m), m)              # and the flag is cleared by a clean call
    assert st == 0 and int(err.item()) == 0
    _same(outs, _reference(dim, k, m), "clean")


@pytest.mark.parametrize("bad_value", [N_ROWS, -2, 2 ** 31 - 1])
def test_a_bad_list_index_poisons_its_own_list_alone(bad_value):
    """out-of-range VALUES, validated before any read: list 21 of 37 becomes -1 / NaN / NaN, the flag is set, the others
    equal the reference"""
    for dim, k, m in ((64, 10, 3), (128, 33, 8)):
        idx, off, hist, w = _case(dim, k, m)
        idx = idx.copy()
        idx[BAD_LIST, k - 1] = bad_value
        _bad_value_round(dim, k, m, (idx, off, hist, w), _poisoned_ref(_reference(dim, k, m), BAD_LIST))


@pytest.mark.parametrize("bad_value", [N_ROWS, -1])
def test_a_bad_history_index_poisons_its_own_list_alone(bad_value):
    for dim, k, m in ((64, 10, 3), (128, 33, 8)):
        idx, off, hist, w = _case(dim, k, m)
        assert off[BAD_LIST + 1] - off[BAD_LIST] >= 2                           # (the last entry of the history is bad)
        hist = hist.copy()
        hist[off[BAD_LIST + 1] - 1] = bad_value
        _bad_value_round(dim, k, m, (idx, off, hist, w), _poisoned_ref(_reference(dim, k, m), BAD_LIST))


def test_a_decreasing_offsets_pair_poisons_its_own_list_alone():
    """offsets[21] past offsets[22]: list 21's pair decreases; list 20 merely reads a longer history (inside the
    arrays: the caller's guarantee), which the restatement follows"""
    for dim, k, m in ((64, 10, 3), (128, 33, 8)):
        idx, off, hist, w = _case(dim, k, m)
        off = off.copy()
        off[BAD_LIST] = off[BAD_LIST + 1] + 3
        assert off[BAD_LIST] <= len(hist) and off[BAD_LIST] > off[BAD_LIST + 1] and off[BAD_LIST] >= off[BAD_LIST - 1]
        ref = _poisoned_ref(E.explain_lists(_table(dim)[2], idx, off, hist, w, m), BAD_LIST)
        _bad_value_round(dim, k, m, (idx, off, hist, w), ref)
    idx, off, hist, w = _case(64, 10, 3)                        # and a negative pair, on the first list
    off = off.copy()
    off[0] = -4
    st, outs, err = _raw(64, (idx, off, hist, w), 3)
    assert st == 0 and int(err.item()) == 1
    _same(outs, _poisoned_ref(_reference(64, 10, 3), 0), "negative offset")


def test_einval_returns_before_writing():
    import torch
    dim, k, m = 128, 20, 3
    case = _case(dim, k, m)
    cases = [dict(dim_arg=48), dict(dim_arg=0), dict(dim_arg=512), dict(n_rows=0), dict(n_rows=-5), dict(n_lists=-1), dict(k=0),
             dict(k=-1), dict(k=129), dict(m=0), dict(m=9), dict(m=-1)]
    cases += [dict(null=n) for n in ("What", "list_idx", "off", "pos", "sim", "contrib", "err")]

    def untouched(tensors):
        return all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in tensors)

    for kw in cases:
        kw = dict(kw)
        st, outs, err = _raw(dim, case, kw.pop("m", m), **kw)
        assert st == -1 and untouched(outs + [err]), kw
    st, outs, err = _raw(256, _case(256, 64, m), m, k=65)       # one past anirec_explain_max_k(256)
    assert st == -1 and untouched(outs + [err])
    st, outs, err = _raw(dim, case, m, n_lists=0)               # no lists: ok, nothing enqueued
    assert st == 0 and untouched(outs + [err])


def test_the_call_is_graph_capturable():
    """captured into a graph the call runs nothing; the replay writes the restatement's bits and clears the flag"""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    for dim, k, m in ((128, 10, 3), (256, 64, 8)):
        Wh = _table(dim)[0]
        idx, off, hist, w = _case(dim, k, m)
        ci, co, ch, cw = _cuda(idx), _cuda(off), _cuda(hist), _cuda(w)
        outs = [poison.fill(torch.empty((N_LISTS, k, m), dtype=dt, device="cuda"), 0x3F)
                for dt in (torch.int32, torch.float32, torch.float32)]
        err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x3F)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            st = lib.anirec_explain_lists(_lib.ptr(Wh), dim, N_ROWS, _lib.ptr(ci), N_LISTS, k, _lib.ptr(co), _lib.ptr(ch),
                                          _lib.ptr(cw), m, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]),
                                          _lib.ptr(err), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        torch.cuda.synchronize()
        assert all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in outs + [err])     # captured, not run
        graph.replay()
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        _same(outs, _reference(dim, k, m), "graph replay")


def test_planted_clusters_explain_their_own():
    """test_listeval_gpu's cluster table — 12 clusters of 8 rows around distinct basis vectors, within-cluster cosines
    >= 0.95 and between-cluster cosines <= 0.2, asserted from the input in float64 — here with one direction shared by
    all the centres (0.4 along the last axis) and noise 0.01, so that the between-cluster cosines are not merely below 0.2
    but close to it (the second half needs 0.1 * own < 1.0 * another, which that table's near-orthogonal clusters, cosines
    around 0, do not give).  List c holds the rows 1 .. 7
    of cluster c; its history is row 0 of every cluster.  With equal weights the top pick of every listed row is its own
    cluster's history row; with the own cluster's weight at 0.1 and the others at 1.0 it is not.  Both inequalities are
    asserted on the float64 cosines with the kernel's error as margin: a cosine is a 32-term fp32 chain of unit rows,
    within 32 * 2**-24 < 1e-5 of the float64 one, rownorm's and the product's rounding included."""
    from anime_recommendations_amd import ops, recs
    rng = np.random.default_rng(0)
    dim, n_cl, per, eps = 32, 12, 8, 1e-5
    centres = np.eye(dim, dtype=np.float32)[:n_cl].copy()
    centres[:, dim - 1] = 0.4
    W = np.repeat(centres, per, axis=0) + rng.normal(0, 0.01, (n_cl * per, dim)).astype(np.float32)
    cluster = np.repeat(np.arange(n_cl), per)
    Wn = W.astype(np.float64) / np.linalg.norm(W.astype(np.float64), axis=1, keepdims=True)
    Cos = Wn @ Wn.T
    same = cluster[:, None] == cluster[None, :]
    print("within-cluster cosine >= %.3f, between-cluster in [%.3f, %.3f]" % (Cos[same].min(), Cos[~same].min(), Cos[~same].max()))
    assert Cos[same].min() >= 0.95 and Cos[~same].max() <= 0.2
    hist_rows = (np.arange(n_cl) * per).astype(np.int32)
    lists = np.stack([c * per + 1 + np.arange(per - 1) for c in range(n_cl)]).astype(np.int32)
    off = np.arange(n_cl + 1, dtype=np.int64) * n_cl
    Wh = ops.rownorm(_cuda(W))
    # equal positive weights: own cluster first
    w_eq = np.full(n_cl * n_cl, 0.8, np.float32)
    for c in range(n_cl):
        for a in lists[c]:
            other = np.delete(Cos[a, hist_rows], c)
            assert 0.8 * (Cos[a, hist_rows[c]] - eps) > 0.8 * (other.max() + eps)
    pos, sim, contrib, hist_row = recs.explain_topk(Wh, _cuda(lists), off, np.tile(hist_rows, n_cl), w_eq, m=3)
    top = hist_row.cpu().numpy()[:, :, 0]
    assert np.array_equal(cluster[top], np.repeat(np.arange(n_cl)[:, None], per - 1, axis=1))
    assert (pos.cpu().numpy()[:, :, 0] == np.arange(n_cl)[:, None]).all() and float(sim[:, :, 0].min()) >= 0.95 - eps
    # the own cluster's rating at 0.1, the others at 1.0: another cluster's row comes first
    w_low = np.ones((n_cl, n_cl), np.float32)
    w_low[np.arange(n_cl), np.arange(n_cl)] = 0.1
    for c in range(n_cl):
        for a in lists[c]:
            other = np.delete(Cos[a, hist_rows], c)
            assert 0.1 * (Cos[a, hist_rows[c]] + eps) < 1.0 * (other.max() - eps), (c, a)
    _, _, _, hist_row = recs.explain_topk(Wh, _cuda(lists), off, np.tile(hist_rows, n_cl), w_low.reshape(-1), m=3)
    top = hist_row.cpu().numpy()[:, :, 0]
    assert (cluster[top] != np.arange(n_cl)[:, None]).all()
    # weight = "similarity" ignores the ratings: own cluster first again
    _, _, c_sim, hist_row = recs.explain_topk(Wh, _cuda(lists), off, np.tile(hist_rows, n_cl), w_low.reshape(-1), m=3,
                                              weight="similarity")
    assert np.array_equal(cluster[hist_row.cpu().numpy()[:, :, 0]], np.repeat(np.arange(n_cl)[:, None], per - 1, axis=1))


# ---- components.explain_recs_frame on a small model ----------------------------------------------------------------
def test_explain_recs_frame(tmp_path):
    import torch
    from anime_recommendations_amd import components as C, data, ops, recs
    model, table = _small_model()
    anime, syn = data.synth_anime_tables(table.anime_ids)
    anime.to_csv(tmp_path / "all_anime.csv", index=False)
    syn.to_csv(tmp_path / "synopses.csv", index=False)
    anime_df, syn_df = C.load_anime_df(tmp_path / "all_anime.csv"), C.load_synopses(tmp_path / "synopses.csv")
    df = pd.DataFrame({"user_id": table.user_ids[table.user], "anime_id": table.anime_ids[table.anime], "rating": table.rating})
    user_row = 4
    user = int(table.user_ids[user_row])
    args = (model["U"], model["A"], HEAD, table.user_ids, table.anime_ids, df, anime_df, syn_df, user, 10)
    plain = C.model_recs_frame(*args)
    frame = C.explain_recs_frame(*args, count=3)
    extra = [c % r for r in (1, 2, 3) for c in ("Because_%d", "Because_%d_rating", "Because_%d_similarity", "Because_%d_contribution")]
    assert frame.columns.tolist() == plain.columns.tolist() + extra and len(frame) == len(plain) == 10
    pd.testing.assert_frame_equal(frame[plain.columns.tolist()], plain, check_exact=True)
    assert np.array_equal(_bits(frame["Prediction"].to_numpy()), _bits(plain["Prediction"].to_numpy()))
    # the reasons, from the layers below: the user's ratings in the frame's order
    mine = df[df.user_id == user]
    assert len(mine) > 20
    meta = C.metadata_by_index(table.anime_ids, anime_df, syn_df)
    listed = pd.Index(table.anime_ids).get_indexer(frame["anime_id"]).astype(np.int32)
    off, hidx, hr = recs.history_csr(table.user, table.anime, table.rating, [user_row])
    assert hidx.tolist() == pd.Index(table.anime_ids).get_indexer(mine.anime_id).tolist()
    What = ops.rownorm(_cuda(np.asarray(model["A"], np.float32)))
    pos, sim, contrib, hist_row = [t.cpu().numpy()[0] for t in recs.explain_topk(What, _cuda(listed[None]), off, hidx, hr, m=3)]
    for r in range(3):
        ok = (pos[:, r] >= 0) & (contrib[:, r] > 0)
        assert ok.any()
        assert frame["Because_%d" % (r + 1)][ok].tolist() == meta["Name"].to_numpy()[hist_row[ok, r]].tolist()
        assert frame["Because_%d" % (r + 1)][~ok].isna().all() and frame["Because_%d_rating" % (r + 1)][~ok].isna().all()
        assert np.array_equal(frame["Because_%d_rating" % (r + 1)][ok].to_numpy(), mine.rating.to_numpy()[pos[ok, r]])
        assert np.array_equal(_bits(frame["Because_%d_similarity" % (r + 1)].to_numpy()[ok]), _bits(sim[ok, r]))
        assert np.array_equal(_bits(frame["Because_%d_contribution" % (r + 1)].to_numpy()[ok]), _bits(contrib[ok, r]))
    # weight = similarity is ops.explain_lists with ones; min_rating drops the low ratings from the reasons
    by_sim = C.explain_recs_frame(*args, count=2, weight="similarity")
    p1, s1, c1 = [t.cpu().numpy()[0] for t in ops.explain_lists(What, _cuda(listed[None]), off, _cuda(hidx),
                                                                   torch.ones(len(hidx), device="cuda"), 2)]
    assert np.array_equal(_bits(c1), _bits(s1)) and (c1 > 0).all()
    for r in range(2):
        assert by_sim["Because_%d" % (r + 1)].tolist() == meta["Name"].to_numpy()[hidx[p1[:, r]]].tolist()
        assert np.array_equal(_bits(by_sim["Because_%d_similarity" % (r + 1)].to_numpy()), _bits(s1[:, r]))
        assert np.array_equal(_bits(by_sim["Because_%d_contribution" % (r + 1)].to_numpy()), _bits(s1[:, r]))
    assert by_sim.columns.tolist() == plain.columns.tolist() + extra[:8]
    high = C.explain_recs_frame(*args, count=3, min_rating=0.7)
    for r in (1, 2, 3):
        col = high["Because_%d_rating" % r]
        assert (col.dropna() >= 0.7).all()
    for kw in (dict(count=0), dict(count=9), dict(weight="both"), dict(min_rating=1.5), dict(min_rating=float("nan"))):
        with pytest.raises(ValueError, match="explain_recs"):
            C.explain_recs_frame(*args, **kw)


# ---- the component, on the pipeline of test_components_gpu.py --------------------------------------------------------
def _flags(user, **extra):
    return dict(main_df="user_stats.parquet:latest", main_df_type="parquet", project_name="anime_recommendations",
                anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopsis_df="synopses.csv:latest",
                sypnopsis_df_type="raw_data", model="wandb_anime_nn.h5:latest", model_type="h5",
                model_user_query=user, random_user=False, model_recs_fn="model_recs.csv", save_model_recs=True,
                model_num_recs=10, anime_types='["TV", "Movie"]', specify_types=True,
                model_genres='["Action", "Comedy", None]', specify_genres=False, model_ID_flow=False,
                model_ID_conf=True, model_recs_type="csv", flow_ID="user_id.csv:latest", flow_ID_type="csv", **extra)


def test_explain_recs_component(pipeline):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, weights_io
    work, env = pipeline["work"], pipeline["env"]
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    user = int(df.user_id.unique()[5])
    m = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest"))
    anime_df = C.load_anime_df(pipeline["paths"]["all_anime"])
    syn_df = C.load_synopses(pipeline["paths"]["synopses"])
    user_ids, anime_ids = C.index_tables(m, df)
    plain = C.model_recs_frame(m["U"], m["A"], weights_io.model_head(m), user_ids, anime_ids, df, anime_df, syn_df, user, 10,
                               types=["TV", "Movie"])
    _run("explain_recs", _flags(user), str(work), env)
    fn = "User_ID_%d_explained_model_recs.csv" % user
    got = pd.read_csv(work / fn)
    reason = ["Because_%d", "Because_%d_rating", "Because_%d_similarity", "Because_%d_contribution"]
    assert got.columns.tolist() == plain.columns.tolist() + [c % r for r in (1, 2, 3) for c in reason]
    assert len(got) == len(plain) == 10 and got["Name"].tolist() == plain["Name"].tolist()
    assert np.array_equal(got["Prediction"].to_numpy().astype(np.float32), plain["Prediction"].to_numpy())
    rated = df[df.user_id == user].merge(anime_df[["anime_id", "Name"]], on="anime_id")
    assert got["Because_1"].notna().all() and set(got["Because_1"]) <= set(rated["Name"])
    assert (got["Because_1_contribution"] >= got["Because_2_contribution"].fillna(0)).all()
    by_name = rated.set_index("Name")["rating"]
    assert np.array_equal(got["Because_1_rating"].to_numpy(), by_name[got["Because_1"]].to_numpy())
    meta = artifacts.artifact_metadata("explained_model_recs.csv:latest")
    assert meta["Filename"] == fn and meta["explain_count"] == 3 and meta["explain_weight"] == "rating"
    assert meta["explain_min_rating"] == 0.0 and meta["Queried user: "] == user
    _run("explain_recs", _flags(user, explain_count=1, explain_weight="similarity", explain_min_rating=0.7), str(work), env)
    one = pd.read_csv(work / fn)
    assert one.columns.tolist() == plain.columns.tolist() + [c % 1 for c in reason] and len(one) == 10
    assert one["Name"].tolist() == plain["Name"].tolist() and (one["Because_1_rating"] >= 0.7).all()
    assert np.array_equal(one["Because_1_similarity"].to_numpy(), one["Because_1_contribution"].to_numpy())
    meta = artifacts.artifact_metadata("explained_model_recs.csv:latest")
    assert meta["explain_count"] == 1 and meta["explain_weight"] == "similarity" and meta["explain_min_rating"] == 0.7
