"""GPU tests of the calibrated re-rank (anirec_calibrate_rerank, anirec_list_calibration, ops.calibrate_rerank,
ops.list_calibration, recs.calibrated_topk, the calibrated_recs component).

Yardstick: the restatement (tests/calibrate_restatement.py).  Every comparison of idx, pos, num, den, the score bits and
the pen bits is exact.

Shapes: n_cat 1, 31, 32, 33, 64, 65, 128 (one to four bit words, full and partial last words); n_cand 1, 63, 64, 65 (a
wave and one past it), 255, 256, 257 (256 is the last list one wave takes, 257 the first of the four-wave workgroup) and
1024 (anirec_calibrate_max_cand()); k 1, min(10, n_cand) and n_cand; calibration 0, 0.1, 0.5 and 1; a 300-row category
table; 8 lists a call, the first of them with the special content ``_lists`` plants.  The re-rank is greedy, so the
reference for k = n_cand is computed once per (n_cat, n_cand, calibration) and its first columns are the reference for
the smaller k.

So that the comparison cannot pass with the penalty ignored, the reference itself is checked first: for calibration
>= 0.1 and n_cat >= 5 every list's full order differs from the score order.  Two kinds of list cannot differ by the
definition, and are left out of that check: the list with the all-zero profile (pen is 0 everywhere) and lists of fewer
than two present candidates (n_cand 1).
"""
import ctypes
import json
import os

import numpy as np
import pandas as pd
import pytest

import calibrate_restatement as R
import poison
from test_components_gpu import _run, pipeline  # noqa: F401  (the components' pipeline fixture, as it is)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, N_LISTS = 300, 8
NO_BITS_ROW = 7                             # a table row without a category
N_CATS = (1, 31, 32, 33, 64, 65, 128)
N_CANDS = (1, 63, 64, 65, 255, 256, 257, 1024)
CALS = (0.0, 0.1, 0.5, 1.0)
ZERO_PROFILE, MAX_ENTRY = 2, 4              # the lists with the all-zero profile and with the entry of exactly 2**24


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_TABLES = {}


def _table(n_cat):
    """uint32 [N_ROWS, cw]: category bits of density min(0.5, 3 / n_cat + 0.02), one row without any, and garbage in the
    bits of the last word at or above n_cat"""
    if n_cat not in _TABLES:
        rng = np.random.default_rng(500 + n_cat)
        cw = (n_cat + 31) // 32
        dense = rng.random((N_ROWS, n_cat)) < min(0.5, 3 / n_cat + 0.02)
        dense[NO_BITS_ROW] = False
        table = np.zeros((N_ROWS, cw), np.uint32)
        for r, c in zip(*np.nonzero(dense)):
            table[r, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
        if n_cat & 31:
            table[:, -1] |= (rng.integers(0, 1 << 32, N_ROWS, dtype=np.uint64).astype(np.uint32)
                             & ~np.uint32((1 << (n_cat & 31)) - 1))
            assert (table[:, -1] >> np.uint32(n_cat & 31)).any()
        assert np.array_equal(R.unpack(table, n_cat), dense)
        _TABLES[n_cat] = table
    return _TABLES[n_cat]


def _lists(n_cat, n_cand, seed=0):
    """N_LISTS candidate lists: random rows, scores of 16 levels sorted descending (ties abound), profile counts below 50,
    the first lists with the content that takes a path of its own, as far as n_cand has room for it."""
    rng = np.random.default_rng(seed * 100000 + n_cat * 2000 + n_cand)
    idx = rng.integers(0, N_ROWS, (N_LISTS, n_cand)).astype(np.int32)
    idx[idx == NO_BITS_ROW] = NO_BITS_ROW + 1
    score = np.sort(rng.integers(0, 16, (N_LISTS, n_cand)).astype(np.float32) / 16, axis=1)[:, ::-1].copy()
    profile = rng.integers(0, 50, (N_LISTS, n_cat)).astype(np.int32)
    mid = n_cand // 2
    idx[0, [0, mid, n_cand - 1]] = -1                           # empty slots at the front, the middle and the end
    score[1, [0, mid]] = np.nan                                 # NaN scores
    profile[ZERO_PROFILE] = 0                                   # nothing to calibrate to
    idx[3, 0] = NO_BITS_ROW                                     # a candidate with no bits (first, at the top score)
    profile[MAX_ENTRY, 0] = 1 << 24                             # the largest entry the definition takes
    if n_cand >= 2:
        idx[5, : n_cand - 1] = -1                               # fewer than k present candidates
    return idx, score, profile


_REFS = {}


def _reference(n_cat, n_cand, cal, seed=0):
    """the restatement for k = n_cand (its first k columns are the reference for any smaller k), once per shape"""
    key = (n_cat, n_cand, cal, seed)
    if key not in _REFS:
        idx, score, profile = _lists(n_cat, n_cand, seed)
        _REFS[key] = R.rerank_lists(_table(n_cat), n_cat, idx, score, profile, n_cand, cal)[:4]
    return _REFS[key]


def _score_order(idx, score):
    """the positions of the present candidates of one list in (score descending, position ascending) order"""
    present = np.flatnonzero((idx >= 0) & ~np.isnan(score))
    return present[np.argsort(-score[present], kind="stable")]


def _penalty_shapes_every_list(n_cat, n_cand, cal, ref, seed=0):
    """the condition of the module docstring, on the reference"""
    idx, score, _ = _lists(n_cat, n_cand, seed)
    for l in range(N_LISTS):
        plain = _score_order(idx[l], score[l])
        if l == ZERO_PROFILE or len(plain) < 2:
            assert ref[1][l, :len(plain)].tolist() == plain.tolist()
        else:
            assert ref[1][l, :len(plain)].tolist() != plain.tolist(), (n_cat, n_cand, cal, l)


def _same(got, ref, k, what):
    gi, gp, gs, gn = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in got]
    assert np.array_equal(gi, ref[0][:, :k]), what
    assert np.array_equal(gp, ref[1][:, :k]), what
    assert np.array_equal(_bits(gs), _bits(ref[2][:, :k])), what
    assert np.array_equal(_bits(gn), _bits(ref[3][:, :k])), what


@pytest.mark.parametrize("cal", CALS)
@pytest.mark.parametrize("n_cand", N_CANDS)
@pytest.mark.parametrize("n_cat", N_CATS)
def test_rerank_equals_the_restatement(n_cat, n_cand, cal):
    from anime_recommendations_amd import ops
    table = _cuda(_table(n_cat).view(np.int32))
    idx, score, profile = _lists(n_cat, n_cand)
    ref = _reference(n_cat, n_cand, cal)
    if cal >= 0.1 and n_cat >= 5:
        _penalty_shapes_every_list(n_cat, n_cand, cal, ref)
    for k in sorted({1, min(10, n_cand), n_cand}):
        got = ops.calibrate_rerank(table, n_cat, _cuda(idx), _cuda(score), _cuda(profile), k, cal)
        _same(got, ref, k, (n_cat, n_cand, k, cal))
    # the planted content did what it is there for (checked on the reference, which the kernel has just equalled)
    ri, rp, rs, rn = ref
    assert (rp[0] >= 0).sum() == max(0, n_cand - len({0, n_cand // 2, n_cand - 1}))
    assert (rp[1] >= 0).sum() == max(0, n_cand - len({0, n_cand // 2}))
    assert (rn[ZERO_PROFILE] == 0).all()
    assert NO_BITS_ROW in ri[3].tolist() and (ri[3] == NO_BITS_ROW).sum() == 1
    if n_cand >= 2:
        assert rp[5, 0] == n_cand - 1 and (rp[5, 1:] == -1).all() and np.isnan(rn[5, 1:]).all()
    if cal == 0.0:
        assert ri[3, 0] == NO_BITS_ROW and rn[3, 0] == 1.0      # the list says nothing after a pick without categories
        assert all(rp[l, :len(o)].tolist() == o.tolist() for l in range(N_LISTS)
                   for o in [_score_order(idx[l], score[l])])


# the shapes the further tests share: a wave's list with a partial second word, a wave's list of every slot a lane owns,
# and the four-wave workgroup
SHAPES = ((43, 100, 10, 0.5), (65, 256, 256, 0.1), (128, 257, 12, 0.5))


@pytest.mark.parametrize("n_cat,n_cand,k,cal", SHAPES + ((1, 20, 20, 1.0), (33, 65, 65, 0.3)))
def test_list_calibration_of_every_prefix_is_out_pen(n_cat, n_cand, k, cal):
    import torch
    from anime_recommendations_amd import ops
    table = _cuda(_table(n_cat).view(np.int32))
    idx, score, profile = _lists(n_cat, n_cand)
    gi, _, _, gpen = ops.calibrate_rerank(table, n_cat, _cuda(idx), _cuda(score), _cuda(profile), k, cal)
    # list (l, s) = the first s + 1 picks of list l
    cols = torch.arange(k, device="cuda")
    prefixes = torch.where(cols[None, None, :] <= cols[None, :, None], gi[:, None, :], torch.full_like(gi[:, None, :], -1))
    pen, num, den = ops.list_calibration(table, n_cat, prefixes.reshape(N_LISTS * k, k),
                                         _cuda(np.repeat(profile, k, axis=0)))
    valid = (gi >= 0).reshape(-1)
    assert int(valid.sum()) > N_LISTS and torch.equal(pen.view(torch.int32)[valid], gpen.reshape(-1).view(torch.int32)[valid])
    want = (num.double() / den.double()).float()
    assert torch.equal(pen.view(torch.int32), want.view(torch.int32)) and bool((num <= den).all()) and bool((num >= 0).all())


@pytest.mark.parametrize("n_cat,k", [(1, 1), (31, 10), (43, 10), (64, 64), (65, 65), (128, 300), (128, 1024)])
def test_list_calibration_equals_the_restatement(n_cat, k):
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(n_cat * 10000 + k)
    n_lists = 40
    lists = rng.integers(0, N_ROWS, (n_lists, k)).astype(np.int32)
    lists[rng.random((n_lists, k)) < 0.3] = -1                  # padding anywhere
    profile = rng.integers(0, 50, (n_lists, n_cat)).astype(np.int32)
    lists[0] = -1                                               # an empty list: 1 / 1
    lists[1] = NO_BITS_ROW                                      # a list without tokens: 1 / 1
    profile[2] = 0                                              # nothing to calibrate to: 0 / 1
    profile[3] = 1 << 24                                        # the largest numerator: every entry 2**24
    lists[3] = rng.integers(0, N_ROWS, k)
    rnum, rden, rpen, err = R.list_calibration(_table(n_cat), n_cat, lists, profile)
    assert err == 0 and (rnum[:3].tolist(), rden[:3].tolist()) == ([1, 1, 0], [1, 1, 1])
    pen, num, den = ops.list_calibration(_cuda(_table(n_cat).view(np.int32)), n_cat, _cuda(lists), _cuda(profile))
    assert np.array_equal(num.cpu().numpy(), rnum) and np.array_equal(den.cpu().numpy(), rden)
    assert np.array_equal(_bits(pen.cpu().numpy()), _bits(rpen))


def test_a_list_does_not_depend_on_its_context():
    """a list run alone, at another position among other lists, and twice: the same bits"""
    from anime_recommendations_amd import ops
    for n_cat, n_cand, k, cal in SHAPES:
        table = _cuda(_table(n_cat).view(np.int32))
        idx, score, profile = _lists(n_cat, n_cand)
        ref = _reference(n_cat, n_cand, cal)
        ci, cs, pr = _cuda(idx), _cuda(score), _cuda(profile)
        _same(ops.calibrate_rerank(table, n_cat, ci, cs, pr, k, cal), ref, k, "whole call")
        _same(ops.calibrate_rerank(table, n_cat, ci, cs, pr, k, cal), ref, k, "second run")
        perm = np.random.default_rng(5).permutation(N_LISTS)
        moved = ops.calibrate_rerank(table, n_cat, _cuda(idx[perm]), _cuda(score[perm]), _cuda(profile[perm]), k, cal)
        _same(moved, [r[perm] for r in ref], k, "permuted call")
        for l in (0, 3, 7):
            alone = ops.calibrate_rerank(table, n_cat, ci[l:l + 1].clone(), cs[l:l + 1].clone(), pr[l:l + 1].clone(), k, cal)
            _same(alone, [r[l:l + 1] for r in ref], k, "list %d alone" % l)


@pytest.mark.parametrize("byte", poison.ORDER)
def test_dirty_outputs_are_fully_overwritten(byte):
    from anime_recommendations_amd import ops
    for n_cat, n_cand, k, cal in SHAPES:
        table = _cuda(_table(n_cat).view(np.int32))
        idx, score, profile = _lists(n_cat, n_cand)
        ci, cs, pr = _cuda(idx), _cuda(score), _cuda(profile)
        log = []
        with poison.poisoned(byte, log):
            got = ops.calibrate_rerank(table, n_cat, ci, cs, pr, k, cal)
        assert len(log) == 5 and sum(log) == 4 * N_LISTS * k * 4 + 4        # the four outputs and the flag word
        ref = _reference(n_cat, n_cand, cal)
        _same(got, ref, k, (byte, n_cat))
        log = []
        with poison.poisoned(byte, log):
            pen, num, den = ops.list_calibration(table, n_cat, got[0], pr)
        assert len(log) == 4 and sum(log) == N_LISTS * (8 + 8 + 4) + 4
        rnum, rden, rpen, _ = R.list_calibration(_table(n_cat), n_cat, ref[0][:, :k], profile)
        assert np.array_equal(num.cpu().numpy(), rnum) and np.array_equal(den.cpu().numpy(), rden)
        assert np.array_equal(_bits(pen.cpu().numpy()), _bits(rpen))


def _raw(n_cat, idx, score, profile, k, cal, n_rows=N_ROWS, n_lists=None, n_cand=None, null=None, fill=0x3F,
         n_cat_arg=None):
    """anirec_calibrate_rerank itself, its outputs and flag pre-filled with ``fill`` bytes: no wrapper check between the
    test and the entry point.  ``null``: the name of one pointer passed as NULL.  Returns (status, outs, err)."""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    shape = (idx.shape[0], max(k, 1))
    outs = [poison.fill(torch.empty(shape, dtype=dt, device="cuda"), fill)
            for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), fill)
    p = dict(cat_bits=_cuda(_table(n_cat).view(np.int32)), cand_idx=_cuda(idx), cand_score=_cuda(score),
             profile=_cuda(profile), out_idx=outs[0], out_pos=outs[1], out_score=outs[2], out_pen=outs[3], err=err)
    if null:
        p[null] = None
    st = lib.anirec_calibrate_rerank(_lib.ptr(p["cat_bits"]), n_rows, n_cat if n_cat_arg is None else n_cat_arg,
                                     _lib.ptr(p["cand_idx"]), _lib.ptr(p["cand_score"]), _lib.ptr(p["profile"]),
                                     idx.shape[0] if n_lists is None else n_lists,
                                     idx.shape[1] if n_cand is None else n_cand, k, cal, _lib.ptr(p["out_idx"]),
                                     _lib.ptr(p["out_pos"]), _lib.ptr(p["out_score"]), _lib.ptr(p["out_pen"]),
                                     _lib.ptr(p["err"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, outs, err


def _raw_list(n_cat, lists, profile, n_rows=N_ROWS, n_lists=None, k=None, null=None, fill=0x3F, n_cat_arg=None):
    """anirec_list_calibration itself, as ``_raw``.  Returns (status, (num, den, pen), err)."""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    outs = [poison.fill(torch.empty(lists.shape[0], dtype=dt, device="cuda"), fill)
            for dt in (torch.int64, torch.int64, torch.float32)]
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), fill)
    p = dict(cat_bits=_cuda(_table(n_cat).view(np.int32)), lists=_cuda(lists), profile=_cuda(profile), out_num=outs[0],
             out_den=outs[1], out_pen=outs[2], err=err)
    if null:
        p[null] = None
    st = lib.anirec_list_calibration(_lib.ptr(p["cat_bits"]), n_rows, n_cat if n_cat_arg is None else n_cat_arg,
                                     _lib.ptr(p["lists"]), _lib.ptr(p["profile"]),
                                     lists.shape[0] if n_lists is None else n_lists, lists.shape[1] if k is None else k,
                                     _lib.ptr(p["out_num"]), _lib.ptr(p["out_den"]), _lib.ptr(p["out_pen"]),
                                     _lib.ptr(p["err"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, outs, err


def _poisoned_list_alone(n_cat, n_cand, k, cal, idx, score, profile, bad_list, what):
    """list ``bad_list`` of both calls is -1 / NaN with the flag set, every other list is the clean reference's"""
    ref = [r.copy() for r in _reference(n_cat, n_cand, cal)]
    ref[0][bad_list], ref[1][bad_list], ref[2][bad_list], ref[3][bad_list] = -1, -1, np.nan, np.nan
    st, outs, err = _raw(n_cat, idx, score, profile, k, cal)
    assert st == 0 and int(err.item()) == 1, what
    _same(outs, ref, k, what)
    lists = np.where(ref[0][:, :k] >= 0, ref[0][:, :k], -1).astype(np.int32)
    lists[bad_list] = idx[bad_list, :k]
    rnum, rden, rpen, rerr = R.list_calibration(_table(n_cat), n_cat, lists, profile)
    assert rerr == 1 and rnum[bad_list] == -1 and rden[bad_list] == -1 and np.isnan(rpen[bad_list])
    st, (num, den, pen), err = _raw_list(n_cat, lists, profile)
    assert st == 0 and int(err.item()) == 1, what
    assert np.array_equal(num.cpu().numpy(), rnum) and np.array_equal(den.cpu().numpy(), rden), what
    assert np.array_equal(_bits(pen.cpu().numpy()), _bits(rpen)), what
    clean = _lists(n_cat, n_cand)                               # and the flag is cleared by a clean call
    st, outs, err = _raw(n_cat, clean[0], clean[1], clean[2], k, cal)
    assert st == 0 and int(err.item()) == 0
    st, _, err = _raw_list(n_cat, lists.clip(-1, N_ROWS - 1), clean[2])
    assert st == 0 and int(err.item()) == 0


@pytest.mark.parametrize("bad_value", [N_ROWS, -2, 2 ** 31 - 1])
@pytest.mark.parametrize("n_cat,n_cand,k,cal", SHAPES[::2])
def test_a_bad_index_poisons_its_own_list_alone(n_cat, n_cand, k, cal, bad_value):
    idx, score, profile = _lists(n_cat, n_cand)
    idx = idx.copy()
    idx[6, k - 1] = bad_value
    _poisoned_list_alone(n_cat, n_cand, k, cal, idx, score, profile, 6, bad_value)


@pytest.mark.parametrize("bad_value", [(1 << 24) + 1, -1, -2 ** 31])
@pytest.mark.parametrize("n_cat,n_cand,k,cal", SHAPES[::2])
def test_a_bad_profile_entry_poisons_its_own_list_alone(n_cat, n_cand, k, cal, bad_value):
    idx, score, profile = _lists(n_cat, n_cand)
    profile = profile.copy()
    profile[6, n_cat - 1] = bad_value
    _poisoned_list_alone(n_cat, n_cand, k, cal, idx, score, profile, 6, bad_value)


def test_einval_returns_before_writing():
    import torch
    n_cat, n_cand, k, cal = 43, 20, 5, 0.5
    idx, score, profile = _lists(n_cat, n_cand)

    def untouched(tensors):
        return all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in tensors)

    cases = [dict(n_cat_arg=0), dict(n_cat_arg=129), dict(n_rows=0), dict(n_lists=-1), dict(n_cand=-1), dict(k=0),
             dict(k=21), dict(n_cand=1025, k=5), dict(cal=-0.01), dict(cal=1.01), dict(cal=float("nan"))]
    cases += [dict(null=n) for n in ("cat_bits", "cand_idx", "cand_score", "profile", "out_idx", "out_pos", "out_score",
                                     "out_pen", "err")]
    for kw in cases:
        st, outs, err = _raw(n_cat, idx, score, profile, **dict(dict(k=k, cal=cal), **kw))
        assert st == -1 and untouched(outs + [err]), kw
    st, outs, err = _raw(n_cat, idx, score, profile, k, cal, n_lists=0)      # no lists: ok, nothing enqueued
    assert st == 0 and untouched(outs + [err])
    cases = [dict(n_cat_arg=0), dict(n_cat_arg=129), dict(n_rows=0), dict(n_lists=-1), dict(k=0), dict(k=1025)]
    cases += [dict(null=n) for n in ("cat_bits", "lists", "profile", "out_num", "out_den", "out_pen", "err")]
    for kw in cases:
        st, outs, err = _raw_list(n_cat, idx, profile, **kw)
        assert st == -1 and untouched(outs + [err]), kw
    st, outs, err = _raw_list(n_cat, idx, profile, n_lists=0)
    assert st == 0 and untouched(outs + [err])


def test_the_calls_are_graph_capturable():
    """captured into a graph the calls run nothing; the replay writes the restatement's bits and clears the flags"""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    n_cat, n_cand, k, cal = SHAPES[0]
    table = _cuda(_table(n_cat).view(np.int32))
    idx, score, profile = _lists(n_cat, n_cand)
    ci, cs, pr = _cuda(idx), _cuda(score), _cuda(profile)
    outs = [poison.fill(torch.empty((N_LISTS, k), dtype=dt, device="cuda"), 0x3F)
            for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
    louts = [poison.fill(torch.empty(N_LISTS, dtype=dt, device="cuda"), 0x3F)
             for dt in (torch.int64, torch.int64, torch.float32)]
    errs = [poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x3F) for _ in range(2)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st = lib.anirec_calibrate_rerank(_lib.ptr(table), N_ROWS, n_cat, _lib.ptr(ci), _lib.ptr(cs), _lib.ptr(pr), N_LISTS,
                                         n_cand, k, cal, *[_lib.ptr(o) for o in outs], _lib.ptr(errs[0]), stream)
        st2 = lib.anirec_list_calibration(_lib.ptr(table), N_ROWS, n_cat, _lib.ptr(outs[0]), _lib.ptr(pr), N_LISTS, k,
                                          *[_lib.ptr(o) for o in louts], _lib.ptr(errs[1]), stream)
    assert st == 0 and st2 == 0
    torch.cuda.synchronize()
    assert all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in outs + louts + errs)     # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert int(errs[0].item()) == 0 and int(errs[1].item()) == 0
    ref = _reference(n_cat, n_cand, cal)
    _same(outs, ref, k, "graph replay")
    last = (ref[0][:, :k] >= 0).sum(axis=1) - 1                 # the list's own figure: the pen of its last pick
    full = last == k - 1
    assert full.sum() >= 6
    assert np.array_equal(_bits(louts[2].cpu().numpy())[full], _bits(ref[3][:, k - 1])[full])


def test_calibration_zero_on_the_pool_is_predict_topk():
    """calibration = 0 on predict_topk(pool) candidates: predict_topk(k), bit for bit"""
    import torch
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(8)
    dim, n_cat, pool, k = 64, 43, 100, 10
    U = _cuda(rng.normal(size=(60, dim)).astype(np.float32))
    A = _cuda(rng.normal(size=(N_ROWS, dim)).astype(np.float32))
    head = dict(w=1.3, b=-0.1, gamma=0.9, beta=0.05, mov_mean=0.02, mov_var=0.8)
    users = np.arange(N_LISTS)
    cand, p = ops.predict_topk(U, A, head, users, pool)
    want_i, want_p = ops.predict_topk(U, A, head, users, k)
    profile = _cuda(_lists(n_cat, pool)[2])
    gi, gpos, gs, _ = ops.calibrate_rerank(_cuda(_table(n_cat).view(np.int32)), n_cat, cand, p, profile, k, 0.0)
    assert torch.equal(gi, want_i) and torch.equal(gs.view(torch.int32), want_p.view(torch.int32))
    assert torch.equal(gpos, torch.arange(k, dtype=torch.int32, device="cuda").expand(N_LISTS, k))


# ---- recs.calibrated_topk and the component, on the pipeline of test_components_gpu.py ------------------------------
def _model():
    from anime_recommendations_amd import artifacts, weights_io
    return weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest"))


def test_calibrated_topk_on_the_trained_model(pipeline):  # noqa: F811
    import torch
    from anime_recommendations_amd import components as C, ops, recs, weights_io
    m = _model()
    U, A, head = _cuda(np.asarray(m["U"], np.float32)), _cuda(np.asarray(m["A"], np.float32)), weights_io.model_head(m)
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    users = np.array([3, 50, 120, 299])
    uid, aid = np.asarray(m["user_ids"]), np.asarray(m["anime_ids"])
    mine = df[df.user_id.isin(uid[users])]
    u_pos = pd.Index(uid[users]).get_indexer(mine.user_id)
    a_pos = pd.Index(aid).get_indexer(mine.anime_id)
    assert (u_pos >= 0).all() and (a_pos >= 0).all()
    watched = ops.seen_bits(u_pos.astype(np.int32), a_pos.astype(np.int32), len(users), len(aid))
    meta = C.metadata_by_index(aid, C.load_anime_df(pipeline["paths"]["all_anime"]))
    names, cat_bits = C.category_table(meta, "Genres")
    n_cat = len(names)
    profile = recs.fave_profile(C.favourite_bits(df, uid, aid, 80), cat_bits, n_cat, users=users)
    assert n_cat >= 2 and bool((profile.sum(dim=1) > 0).all())
    k, pool = 10, 100
    # calibration 0: ops.predict_topk itself
    gi, gp, gpen = recs.calibrated_topk(U, A, head, users, k, pool, 0.0, cat_bits, n_cat, profile, watched)
    wi, wp = ops.predict_topk(U, A, head, users, k, watched)
    assert gpen is None and torch.equal(gi, wi) and torch.equal(gp.view(torch.int32), wp.view(torch.int32))
    plain = recs.list_calibration(wi, cat_bits, n_cat, profile)[0].cpu().numpy()
    # calibration 0.5: the restatement on the pool list, several users at once, under the watched mask
    gi, gp, gpen = recs.calibrated_topk(U, A, head, users, k, pool, 0.5, cat_bits, n_cat, profile, watched)
    cand, p = ops.predict_topk(U, A, head, users, pool, watched)
    ri, _, rs, rn, err = R.rerank_lists(cat_bits, n_cat, cand.cpu().numpy(), p.cpu().numpy(), profile.cpu().numpy(), k, 0.5)
    assert err == 0 and np.array_equal(gi.cpu().numpy(), ri) and np.array_equal(_bits(gp.cpu().numpy()), _bits(rs))
    assert np.array_equal(_bits(gpen.cpu().numpy()), _bits(rn))
    figure = gpen.cpu().numpy()[:, -1]
    print("miscalibration of the top-%d: plain %s, calibrated %s" % (k, plain.tolist(), figure.tolist()))
    assert (figure <= plain).all()                              # the list's own figure is not above the plain top-k's
    assert np.array_equal(_bits(recs.list_calibration(gi, cat_bits, n_cat, profile)[0].cpu().numpy()), _bits(figure))
    for r in range(len(users)):                                 # nothing watched is listed
        assert not (set(aid[gi.cpu().numpy()[r]].tolist()) & set(df[df.user_id == uid[users[r]]].anime_id))
    # a pool beyond the table is clamped to it
    ci, cp, _ = recs.calibrated_topk(U, A, head, users, k, 10 ** 6 if len(aid) <= 1024 else 1024, 0.5, cat_bits, n_cat,
                                     profile)
    assert tuple(ci.shape) == (len(users), k) and bool((ci >= 0).all())


def test_calibrated_recs_component(pipeline, golden_dir):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, recs, weights_io
    work, env = pipeline["work"], pipeline["env"]
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    user = int(df.user_id.unique()[5])
    m = _model()
    anime_df = C.load_anime_df(pipeline["paths"]["all_anime"])
    syn_df = C.load_synopses(pipeline["paths"]["synopses"])
    user_ids, anime_ids = C.index_tables(m, df)
    fmt = json.load(open(os.path.join(golden_dir, "reference_output_formats.json")))["User_ID_153695_model_recs.csv"]
    meta = C.metadata_by_index(anime_ids, anime_df, syn_df)
    frames = {}
    for calibration, column in ((0.5, "Source"), (0, "Genres")):
        flags = dict(main_df="user_stats.parquet:latest", main_df_type="parquet", project_name="anime_recommendations",
                     anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopsis_df="synopses.csv:latest",
                     sypnopsis_df_type="raw_data", model="wandb_anime_nn.h5:latest", model_type="h5",
                     model_user_query=user, random_user=False, model_recs_fn="model_recs.csv", save_model_recs=True,
                     model_num_recs=10, anime_types='["TV", "Movie"]', specify_types=True,
                     model_genres='["Action", "Comedy", None]', specify_genres=False, model_ID_flow=False,
                     model_ID_conf=True, model_recs_type="csv", flow_ID="user_id.csv:latest", flow_ID_type="csv",
                     calibration=calibration, pool=60, calibration_column=column)
        _run("calibrated_recs", flags, str(work), env)
        got = pd.read_csv(work / ("User_ID_%d_calibrated_model_recs.csv" % user))
        assert got.columns.tolist() == fmt["columns"] + ["Miscalibration"] and len(got) == fmt["n_rows"]
        want, stats = C.calibrated_recs_frame(m["U"], m["A"], weights_io.model_head(m), user_ids, anime_ids, df, anime_df,
                                              syn_df, user, 10, types=["TV", "Movie"], pool=60, calibration=calibration,
                                              column=column)
        assert got["anime_id"].tolist() == want["anime_id"].tolist() and got["Name"].tolist() == want["Name"].tolist()
        for col in ("Prediction", "Miscalibration"):
            assert np.array_equal(got[col].to_numpy().astype(np.float32), want[col].to_numpy().astype(np.float32)), col
        assert got["Type"].isin(["TV", "Movie"]).all() and not (set(got["anime_id"]) & set(df[df.user_id == user].anime_id))
        # the Miscalibration column is list_calibration of the prefixes
        names, cat_bits = C.category_table(meta, column)
        u = C.user_index(user_ids, user)
        profile = recs.fave_profile(C.favourite_bits(df, user_ids, anime_ids, 80), cat_bits, len(names), users=[u])
        rows = pd.Index(np.asarray(anime_ids)).get_indexer(got["anime_id"].to_numpy()).astype(np.int32)
        lists = np.where(np.arange(10)[None, :] <= np.arange(10)[:, None], rows[None, :], -1).astype(np.int32)
        pen = recs.list_calibration(_cuda(lists), cat_bits, len(names), profile.expand(10, len(names)))[0].cpu().numpy()
        assert np.array_equal(_bits(pen), _bits(got["Miscalibration"].to_numpy().astype(np.float32)))
        md = artifacts.artifact_metadata("calibrated_model_recs.csv:latest")
        assert {"calibration", "pool", "column", "n_favourites", "miscalibration", "miscalibration_topk", "Filename",
                "Queried user: "} <= set(md)
        assert (md["calibration"], md["pool"], md["column"]) == (calibration, 60, column) and md["n_favourites"] >= 1
        assert np.float32(md["miscalibration"]) == np.float32(stats["miscalibration"]) == np.float32(got["Miscalibration"].iloc[-1])
        assert md["miscalibration_topk"] == stats["miscalibration_topk"]
        frames[(calibration, column)] = (got, stats)
    plain = C.model_recs_frame(m["U"], m["A"], weights_io.model_head(m), user_ids, anime_ids, df, anime_df, syn_df, user,
                               10, types=["TV", "Movie"])
    got0, stats0 = frames[(0, "Genres")]
    assert got0["anime_id"].tolist() == plain["anime_id"].tolist()
    assert np.array_equal(got0["Prediction"].to_numpy().astype(np.float32), plain["Prediction"].to_numpy())
    assert stats0["miscalibration"] == stats0["miscalibration_topk"]
    _, stats5 = C.calibrated_recs_frame(m["U"], m["A"], weights_io.model_head(m), user_ids, anime_ids, df, anime_df, syn_df,
                                        user, 10, types=["TV", "Movie"], pool=60, calibration=0.5, column="Genres")
    assert stats5["miscalibration_topk"] == stats0["miscalibration"] and stats5["miscalibration"] <= 1.0
