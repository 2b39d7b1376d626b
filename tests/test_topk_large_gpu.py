"""Exact top-k for any k (anirec_cosine_topk_large / anirec_predict_topk_large_act) on the GPU.

Every list is held, bitwise in index and score, to oracle.anirec_oracle.topk_desc applied to the GPU's own score
rows (ops.cosine_scores, ops.predict_grid): score descending, ties ascending index, NaN last, -1 / NaN padding.
The k values straddle the one-workgroup LDS sort (k <= 20480) and the tiled sort with merge passes above it; the
tables hold exact duplicate rows (ties) across slice and sort-tile boundaries and zero rows (NaN scores)."""
import ctypes as C
import datetime
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import anirec_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = np.uint32(0x7FC00000)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _table(n, seed):
    """n x 128 rows: random, plus copies of row 7 at slice (2048-ish) and sort-tile (16384) boundaries and at random
    places, plus zero rows (NaN after the NumPy row norm) spread over the table."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((n, 128)).astype(np.float32)
    dup = [p for b in (2048, 2344, 16384) for m in range(1, n // b + 1) for p in (m * b - 1, m * b) if p < n]
    dup = sorted(set(dup) | set(rng.choice(n, min(40, n // 10), replace=False).tolist()) - {7})
    W[dup] = W[7]
    zero = rng.choice(np.setdiff1d(np.arange(n), dup + [7]), max(3, n // 500), replace=False)
    W[zero] = 0.0
    return W, np.asarray(dup), zero


def _queries(n, nq, dup, zero, seed):
    rng = np.random.default_rng(seed)
    q = rng.choice(n, nq, replace=False)
    q[0] = 7                                   # its copies tie with it (and with each other) in every list
    if nq > 1:
        q[1] = zero[0]                         # an all-NaN score row
    if nq > 2:
        q[2] = dup[len(dup) // 2]
    return q.astype(np.int32)


def _expected(order, k):
    """first k of a full oracle ranking (idx, scores), padded to k"""
    ii, ss = order
    oi = np.full(k, -1, np.int64)
    os_ = np.full(k, NAN_BITS, np.uint32)
    m = min(k, len(ii))
    oi[:m] = ii[:m]
    os_[:m] = _bits(ss[:m])
    return oi, os_


def _check(gi, gs, orders, k, tag):
    gi, gs = gi.cpu().numpy(), _bits(gs.cpu().numpy())
    assert gi.shape == (len(orders), k), tag
    for r, order in enumerate(orders):
        ei, es = _expected(order, k)
        assert np.array_equal(gi[r], ei), (tag, r, np.nonzero(gi[r] != ei)[0][:5])
        assert np.array_equal(gs[r], es), (tag, r)


def _large_cosine(lib, Wh, q, k, keep=None, exclude_self=True):
    """anirec_cosine_topk_large called directly (any k, k <= 128 included)"""
    from anime_recommendations_amd import _lib
    dev = Wh.device
    n, nq = Wh.shape[0], len(q)
    qt = torch.as_tensor(q, dtype=torch.int32, device=dev)
    kt = None if keep is None else torch.as_tensor(keep, dtype=torch.uint8, device=dev)
    oi = torch.empty(nq, k, dtype=torch.int32, device=dev)
    os_ = torch.empty(nq, k, dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.anirec_topk_large_workspace_bytes(n, nq, k)), dtype=torch.uint8, device=dev)
    _lib.check(lib.anirec_cosine_topk_large(_lib.ptr(Wh), n, _lib.ptr(qt), nq, _lib.ptr(kt), int(exclude_self), k,
                                            _lib.ptr(oi), _lib.ptr(os_), _lib.ptr(ws), ws.numel(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "anirec_cosine_topk_large")
    return oi, os_


@pytest.mark.parametrize("n", [1000, 17560, 150000])
@pytest.mark.parametrize("nq", [1, 3, 300])
def test_cosine_topk_any_k_equals_the_oracle_ranking(n, nq):
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    W, dup, zero = _table(n, seed=n + nq)
    Wh = ops.rownorm(torch.from_numpy(W))
    q = _queries(n, nq, dup, zero, seed=nq)
    keep = np.random.default_rng(5).random(n) < 0.9
    variants = [(keep, True), (None, False)] if nq == 1 else [(keep if nq == 300 else None, nq != 3)]
    rows = [ops.cosine_scores(Wh, int(x)).cpu().numpy() for x in q]
    for mask, excl in variants:
        orders = [orc.topk_desc(s, n + 5, exclude=int(x) if excl else None, mask=mask) for s, x in zip(rows, q)]
        if mask is None and not excl:
            assert any(np.isnan(o[1][:n]).any() for o in orders)          # NaN scores inside k = n
        ref_i, ref_s = ops.cosine_topk(Wh, q, 128, exclude_self=excl, keep=mask)
        for k in (129, 1000, 16384, 20481, n - 1, n, n + 5):
            gi, gs = ops.cosine_topk(Wh, q, k, exclude_self=excl, keep=mask)
            tag = (n, nq, k, mask is not None, excl)
            _check(gi, gs, orders, k, tag)
            assert torch.equal(gi[:, :128], ref_i) and np.array_equal(_bits(gs[:, :128].cpu()), _bits(ref_s.cpu())), tag
        if n == 17560:
            for k in (1, 10, 100, 128):                     # the new entry point at small k: the existing kernel's lists
                li, ls = _large_cosine(lib, Wh, q, k, keep=mask, exclude_self=excl)
                si, ss = ops.cosine_topk(Wh, q, k, exclude_self=excl, keep=mask)
                assert torch.equal(li, si) and np.array_equal(_bits(ls.cpu()), _bits(ss.cpu())), (k, nq)


def test_cosine_topk_large_rejects_bad_k_and_small_workspace():
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    Wh = ops.rownorm(torch.from_numpy(_table(3000, 1)[0]))
    with pytest.raises(ValueError):
        ops.cosine_topk(Wh, [0], 0)
    q = torch.zeros(1, dtype=torch.int32, device=Wh.device)
    out = torch.empty(4096, dtype=torch.int64, device=Wh.device)
    need = int(lib.anirec_topk_large_workspace_bytes(3000, 1, 4096))
    assert need > int(lib.anirec_topk_large_workspace_bytes(3000, 1, 129))
    ws = torch.empty(need - 1, dtype=torch.uint8, device=Wh.device)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.anirec_cosine_topk_large(_lib.ptr(Wh), 3000, _lib.ptr(q), 1, None, 1, 4096, _lib.ptr(out),
                                        _lib.ptr(out), _lib.ptr(ws), ws.numel(), s) == -3       # ANIREC_EWORKSPACE
    assert lib.anirec_cosine_topk_large(_lib.ptr(Wh), 3000, _lib.ptr(q), 1, None, 1, 0, _lib.ptr(out),
                                        _lib.ptr(out), _lib.ptr(ws), ws.numel(), s) == -1       # ANIREC_EINVAL
    # the existing entry point keeps its limit
    ws2 = torch.empty(int(lib.anirec_topk_workspace_bytes(3000, 1)), dtype=torch.uint8, device=Wh.device)
    assert lib.anirec_cosine_topk(_lib.ptr(Wh), 3000, _lib.ptr(q), 1, None, 1, 129, _lib.ptr(out), _lib.ptr(out),
                                  _lib.ptr(ws2), ws2.numel(), s) == -1


# ---- predict ----------------------------------------------------------------------------------------------------
N_ANIME = 17560
# heads with flat regions: relu at y <= 0 for most anime, sigmoid / tanh saturated to exactly 1 (and 0 / -1)
PRED_HEADS = {"sigmoid": dict(w=60.0, b=0.0, gamma=1.0, beta=8.0, mov_mean=0.0, mov_var=1.0),
              "linear": dict(w=1.3, b=0.1, gamma=0.9, beta=0.5, mov_mean=0.05, mov_var=0.8),
              "tanh": dict(w=40.0, b=0.0, gamma=1.0, beta=3.0, mov_mean=0.0, mov_var=1.0),
              "relu": dict(w=2.0, b=0.0, gamma=1.0, beta=-0.3, mov_mean=0.2, mov_var=0.6),
              "softplus": dict(w=-2.5, b=0.0, gamma=1.0, beta=0.4, mov_mean=0.0, mov_var=0.7)}


def _predict_tables(n_users):
    rng = np.random.default_rng(11)
    U = rng.standard_normal((n_users, 128)).astype(np.float32)
    A = rng.standard_normal((N_ANIME, 128)).astype(np.float32)
    A[[100, 16383, 16384, 17000]] = A[5]                  # equal ratings at the sort-tile boundary
    return U, A


def _watched(nq, seed):
    rng = np.random.default_rng(seed)
    w = rng.random((nq, N_ANIME)) < 0.3
    bits = np.zeros((nq, (N_ANIME + 31) // 32), np.uint32)
    for r in range(nq):
        nz = np.nonzero(w[r])[0]
        np.bitwise_or.at(bits[r], nz >> 5, np.uint32(1) << (nz & 31).astype(np.uint32))
    return w, bits


@pytest.mark.parametrize("act", sorted(PRED_HEADS))
@pytest.mark.parametrize("nq", [1, 257])
def test_predict_topk_any_k_equals_the_oracle_ranking(act, nq):
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    head = dict(PRED_HEADS[act], activation=act)
    U, A = _predict_tables(300)
    tU, tA = torch.from_numpy(U).cuda(), torch.from_numpy(A).cuda()
    users = np.random.default_rng(nq).choice(300, nq, replace=False).astype(np.int32)
    w, bits = _watched(nq, seed=nq + 1)
    grid = ops.predict_grid(tU, tA, head, users).cpu().numpy()
    flat = {"relu": 0.0, "sigmoid": 1.0, "tanh": 1.0}.get(act)
    if flat is not None:                                   # the head really has a flat region
        assert (grid == np.float32(flat)).sum() > nq * 100, act
    orders = [orc.topk_desc(grid[r], N_ANIME + 1, mask=~w[r]) for r in range(nq)]
    ref_i, ref_p = ops.predict_topk(tU, tA, head, users, 128, bits.view(np.int32))
    for k in (129, 5000, N_ANIME):
        gi, gp = ops.predict_topk(tU, tA, head, users, k, bits.view(np.int32))
        _check(gi, gp, orders, k, (act, nq, k))
        assert torch.equal(gi[:, :128], ref_i) and np.array_equal(_bits(gp[:, :128].cpu()), _bits(ref_p.cpu()))
    # without a watched mask: every anime is a candidate
    gi, gp = ops.predict_topk(tU, tA, head, users, N_ANIME)
    _check(gi, gp, [orc.topk_desc(grid[r], N_ANIME) for r in range(nq)], N_ANIME, (act, nq, "all"))
    # the new entry point at small k equals anirec_predict_topk_act
    dev = tU.device
    us = torch.as_tensor(users, device=dev)
    wb = torch.as_tensor(bits.view(np.int32), device=dev)
    h = ops._head_struct(head)
    for k in (1, 10, 100, 128):
        oi = torch.empty(nq, k, dtype=torch.int32, device=dev)
        op = torch.empty(nq, k, dtype=torch.float32, device=dev)
        ws = torch.empty(int(lib.anirec_predict_topk_large_workspace_bytes(N_ANIME, nq, k)), dtype=torch.uint8,
                         device=dev)
        _lib.check(lib.anirec_predict_topk_large_act(_lib.ptr(tU), _lib.ptr(tA), N_ANIME, _lib.ptr(us), nq,
                                                     C.byref(h), ops._head_act(head), _lib.ptr(wb), k, _lib.ptr(oi),
                                                     _lib.ptr(op), _lib.ptr(ws), ws.numel(),
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "anirec_predict_topk_large_act")
        si, sp = ops.predict_topk(tU, tA, head, users, k, bits.view(np.int32))
        assert torch.equal(oi, si) and np.array_equal(_bits(op.cpu()), _bits(sp.cpu())), (act, k)


def test_predict_topk_rejects_k_below_one():
    from anime_recommendations_amd import ops
    U, A = _predict_tables(4)
    with pytest.raises(ValueError):
        ops.predict_topk(torch.from_numpy(U).cuda(), torch.from_numpy(A).cuda(), PRED_HEADS["linear"], [0], 0)


# ---- the batch loop, the merge pass and the slicing boundary of the four exact entry points -------------------------
EWORKSPACE = -3


def _cosine_w(lib, large, Wh, q, k, keep, ws_bytes):
    """anirec_cosine_topk_w / anirec_cosine_topk_large_w on a workspace of exactly ws_bytes: status, idx, scores"""
    from anime_recommendations_amd import _lib
    dev, (n, dim), nq = Wh.device, Wh.shape, len(q)
    qt = torch.as_tensor(q, dtype=torch.int32, device=dev)
    kt = None if keep is None else torch.as_tensor(keep, dtype=torch.uint8, device=dev)
    oi = torch.empty(nq, k, dtype=torch.int32, device=dev)
    os_ = torch.empty(nq, k, dtype=torch.float32, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    fn = lib.anirec_cosine_topk_large_w if large else lib.anirec_cosine_topk_w
    st = fn(_lib.ptr(Wh), n, dim, _lib.ptr(qt), nq, _lib.ptr(kt), 1, k, _lib.ptr(oi), _lib.ptr(os_), _lib.ptr(ws),
            ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return st, oi, os_


def _predict_w(lib, large, tU, tA, head, users, bits, k, ws_bytes):
    """anirec_predict_topk_w / anirec_predict_topk_large_w on a workspace of exactly ws_bytes: status, idx, ratings"""
    from anime_recommendations_amd import _lib, ops
    dev, (n, dim), nq = tU.device, tA.shape, len(users)
    us = torch.as_tensor(users, dtype=torch.int32, device=dev)
    wb = torch.as_tensor(bits.view(np.int32), device=dev)
    oi = torch.empty(nq, k, dtype=torch.int32, device=dev)
    op = torch.empty(nq, k, dtype=torch.float32, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    h = ops._head_struct(head)
    fn = lib.anirec_predict_topk_large_w if large else lib.anirec_predict_topk_w
    st = fn(_lib.ptr(tU), _lib.ptr(tA), dim, n, _lib.ptr(us), nq, C.byref(h), ops._head_act(head), _lib.ptr(wb), k,
            _lib.ptr(oi), _lib.ptr(op), _lib.ptr(ws), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return st, oi, op


def _bit_rows(w):
    bits = np.zeros((w.shape[0], (w.shape[1] + 31) // 32), np.uint32)
    for r in range(w.shape[0]):
        nz = np.nonzero(w[r])[0]
        np.bitwise_or.at(bits[r], nz >> 5, np.uint32(1) << (nz & 31).astype(np.uint32))
    return bits


@pytest.mark.parametrize("width", [128, 32])
@pytest.mark.parametrize("n", [300, 4100])                 # one workgroup per query; two slices and the merge pass
def test_batch_loop_gives_the_same_lists_on_the_smallest_workspace(n, width):
    """The four _w entry points with nq = 5, once on the workspace of their size function (one batch) and once on the
    smallest they take (fixed part + one query: five trips through the batch loop, the masks and outputs advancing with
    the batch): the same lists and score bits, the oracle's; one byte less is refused."""
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    nq = 5
    rng = np.random.default_rng(n + width)
    W = rng.standard_normal((n, width)).astype(np.float32)
    W[[11, n // 2, n - 1]] = W[3]                          # ties, across the slice boundary at 4100
    Wh = ops.rownorm(torch.from_numpy(W))
    q = np.array([3, n - 1, 17, n // 2 + 1, 200], np.int32)
    keep = rng.random(n) < 0.8
    rows = [ops.cosine_scores(Wh, int(x)).cpu().numpy() for x in q]
    # nq = 1 and nq = 5 have the same 256-byte self[] head: the smallest workspace is the size of a one-query call
    for large, k, full, least in ((False, 7, lib.anirec_topk_workspace_bytes(n, nq),
                                   lib.anirec_topk_workspace_bytes(n, 1)),
                                  (True, 7, lib.anirec_topk_large_workspace_bytes(n, nq, 7),
                                   lib.anirec_topk_large_workspace_bytes(n, 1, 7)),
                                  (True, 200, lib.anirec_topk_large_workspace_bytes(n, nq, 200),
                                   lib.anirec_topk_large_workspace_bytes(n, 1, 200))):
        orders = [orc.topk_desc(s, k, exclude=int(x), mask=keep) for s, x in zip(rows, q)]
        assert least < full
        for nb in (full, least):
            st, gi, gs = _cosine_w(lib, large, Wh, q, k, keep, int(nb))
            assert st == 0, (large, k, nb)
            _check(gi, gs, orders, k, ("cosine", n, width, large, k, nb == least))
        assert _cosine_w(lib, large, Wh, q, k, keep, int(least) - 1)[0] == EWORKSPACE

    head = dict(PRED_HEADS["tanh"], activation="tanh")
    tU = torch.from_numpy(rng.standard_normal((40, width)).astype(np.float32)).cuda()
    A = rng.standard_normal((n, width)).astype(np.float32)
    A[[11, n // 2, n - 1]] = A[3]
    tA = torch.from_numpy(A).cuda()
    users = np.array([7, 0, 39, 21, 8], np.int32)
    w = rng.random((nq, n)) < 0.3
    bits = _bit_rows(w)
    grid = ops.predict_grid(tU, tA, head, users).cpu().numpy()
    # the head of a predict workspace holds a normalised row per user of the call: four more than a one-user call
    more = 4 * width * 4
    for large, k, full, least in ((False, 7, lib.anirec_predict_workspace_bytes_w(n, nq, 1, width),
                                   lib.anirec_predict_workspace_bytes_w(n, 1, 1, width) + more),
                                  (True, 7, lib.anirec_predict_topk_large_workspace_bytes_w(n, nq, 7, width),
                                   lib.anirec_predict_topk_large_workspace_bytes_w(n, 1, 7, width) + more),
                                  (True, 200, lib.anirec_predict_topk_large_workspace_bytes_w(n, nq, 200, width),
                                   lib.anirec_predict_topk_large_workspace_bytes_w(n, 1, 200, width) + more)):
        orders = [orc.topk_desc(grid[r], k, mask=~w[r]) for r in range(nq)]
        assert least < full
        for nb in (full, least):
            st, gi, gp = _predict_w(lib, large, tU, tA, head, users, bits, k, int(nb))
            assert st == 0, (large, k, nb)
            _check(gi, gp, orders, k, ("predict", n, width, large, k, nb == least))
        assert _predict_w(lib, large, tU, tA, head, users, bits, k, int(least) - 1)[0] == EWORKSPACE


def test_short_slice_goes_through_the_merge_pass():
    """n = 4100, one query, k = 128: two slices of 2050 keys.  The second slice holds 50 candidates (fewer than k: its
    winners list is short and padded), two of them copies of a row of the first slice, so equal scores meet in the merge
    pass.  With 60 candidates in all the merged row is shorter than k: -1 / NaN from column 60 on."""
    from anime_recommendations_amd import ops
    n, k, half = 4100, 128, 2050
    rng = np.random.default_rng(41)
    W = rng.standard_normal((n, 128)).astype(np.float32)
    second = half + rng.choice(half, 50, replace=False)
    copies = np.sort(second[:2])
    W[copies] = W[100]                                      # row 100 is in the first slice and is kept below
    W[9] = W[100] + 0.05 * rng.standard_normal(128).astype(np.float32)   # a query whose list starts with the three
    Wh = ops.rownorm(torch.from_numpy(W))
    first10 = np.array([100, 5, 77, 640, 1200, 1999, 2000, 2047, 2048, 2049])
    for first in (np.arange(half), first10):                # 2050 + 50 candidates; 10 + 50
        keep = np.zeros(n, bool)
        keep[first] = True
        keep[second] = True
        for q in (100, 9):                                  # the copies tie with each other; with row 100 itself too
            row = ops.cosine_scores(Wh, q).cpu().numpy()
            order = orc.topk_desc(row, k, exclude=q, mask=keep)
            m = int(keep.sum()) - int(keep[q])
            assert len(order[0]) == min(k, m)
            tied = ([100] if q == 9 else []) + copies.tolist()          # equal scores from both slices lead the list
            assert order[0][:len(tied)].tolist() == tied
            gi, gs = ops.cosine_topk(Wh, [q], k, keep=keep)
            _check(gi, gs, [order], k, ("short slice", len(first), q))
            if m < k:
                assert (gi.cpu().numpy()[0, m:] == -1).all() and (_bits(gs.cpu().numpy())[0, m:] == NAN_BITS).all()


def test_slicing_boundary_both_sides_equal_the_oracle():
    """The select is sliced for nq < 1024 and n >= 4096: n = 4095 | 4096 at nq = 1 and nq = 1023 | 1024 at n = 4096,
    k = 10.  Each side equals the oracle, and the any-k entry point at the same shape equals the <= 128 one."""
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    k = 10
    W, dup, zero = _table(4096, seed=12)
    keep = np.random.default_rng(6).random(4096) < 0.9
    for n in (4095, 4096):
        Wh = ops.rownorm(torch.from_numpy(W[:n]))
        q = np.array([7], np.int32)
        order = orc.topk_desc(ops.cosine_scores(Wh, 7).cpu().numpy(), k, exclude=7, mask=keep[:n])
        gi, gs = ops.cosine_topk(Wh, q, k, keep=keep[:n])
        _check(gi, gs, [order], k, ("boundary n", n))
        li, ls = _large_cosine(lib, Wh, q, k, keep=keep[:n])
        assert torch.equal(li, gi) and np.array_equal(_bits(ls.cpu()), _bits(gs.cpu())), n
    Wh = ops.rownorm(torch.from_numpy(W))
    q = _queries(4096, 1024, dup, zero, seed=3)
    orders = [orc.topk_desc(ops.cosine_scores(Wh, int(x)).cpu().numpy(), k, exclude=int(x), mask=keep) for x in q]
    for nq in (1023, 1024):
        gi, gs = ops.cosine_topk(Wh, q[:nq], k, keep=keep)
        _check(gi, gs, orders[:nq], k, ("boundary nq", nq))
        li, ls = _large_cosine(lib, Wh, q[:nq], k, keep=keep)
        assert torch.equal(li, gi) and np.array_equal(_bits(ls.cpu()), _bits(gs.cpu())), nq


# ---- sharded: world 1 and gloo world 2 sharing one GPU --------------------------------------------------------------
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _shard_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    try:
        from anime_recommendations_amd import dist_infer, ops
        torch.cuda.set_device(0)
        W, _, _ = _table(2500, 3)
        Wh = ops.rownorm(torch.from_numpy(W))
        keep = np.random.default_rng(2).random(2500) < 0.8
        ci, cs = dist_infer.sharded_cosine_topk(Wh, 300, keep=keep)
        U, A = _predict_tables(301)
        _, bits = _watched(301, seed=9)
        head = dict(PRED_HEADS["sigmoid"], activation="sigmoid")
        pi, pp = dist_infer.sharded_predict_topk(torch.from_numpy(U).cuda(), torch.from_numpy(A).cuda(), head,
                                                 np.arange(301, dtype=np.int32), 300, bits.view(np.int32))
        torch.cuda.synchronize()
        if rank == 0:
            np.savez(os.path.join(out_dir, "w%d.npz" % world), ci=ci.cpu().numpy(), cs=cs.cpu().numpy(),
                     pi=pi.cpu().numpy(), pp=pp.cpu().numpy())
    finally:
        dist.destroy_process_group()


def test_sharded_large_k_equals_the_single_call(tmp_path):
    from anime_recommendations_amd import ops
    for world in (1, 2):
        mp.spawn(_shard_worker, args=(world, _port(), str(tmp_path)), nprocs=world, join=True)
    W, _, _ = _table(2500, 3)
    Wh = ops.rownorm(torch.from_numpy(W))
    keep = np.random.default_rng(2).random(2500) < 0.8
    si, ss = ops.cosine_topk(Wh, np.arange(2500), 300, keep=keep)
    U, A = _predict_tables(301)
    _, bits = _watched(301, seed=9)
    head = dict(PRED_HEADS["sigmoid"], activation="sigmoid")
    pi, pp = ops.predict_topk(torch.from_numpy(U).cuda(), torch.from_numpy(A).cuda(), head, np.arange(301), 300,
                              bits.view(np.int32))
    for world in (1, 2):
        d = np.load(tmp_path / ("w%d.npz" % world))
        assert np.array_equal(d["ci"], si.cpu().numpy()) and np.array_equal(_bits(d["cs"]), _bits(ss.cpu())), world
        assert np.array_equal(d["pi"], pi.cpu().numpy()) and np.array_equal(_bits(d["pp"]), _bits(pp.cpu())), world


# ---- components, on the pipeline of test_components_gpu.py ---------------------------------------------------------
def _run(comp, flags, cwd, env):
    argv = [sys.executable, os.path.join(ROOT, comp, comp + ".py")]
    for k, v in flags.items():
        argv += ["--" + k, str(v)]
    r = subprocess.run(argv, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return r.stdout.decode()


@pytest.fixture(scope="module")
def pipeline(tmp_path_factory):
    from anime_recommendations_amd import artifacts, data
    work = tmp_path_factory.mktemp("pipe")
    env = dict(os.environ, ANIREC_ARTIFACT_DIR=str(work / "store"), ANIREC_SEED="3")
    os.environ["ANIREC_ARTIFACT_DIR"] = env["ANIREC_ARTIFACT_DIR"]
    paths = data.write_synthetic_dataset(str(work / "data"), n_users=300, n_anime=500, n_ratings=40_000, seed=2)
    artifacts.log_artifact("user_stats.parquet", paths["user_stats"], "parquet")
    artifacts.log_artifact("all_anime.csv", paths["all_anime"], "raw_data")
    artifacts.log_artifact("synopses.csv", paths["synopses"], "raw_data")
    nn = dict(test_size=2000, TPU_INIT=False, embedding_size=128, kernel_initializer="he_normal",
              activation_function="sigmoid", model_loss="binary_crossentropy", optimizer="Adam",
              start_lr=1e-4, min_lr=1e-4, max_lr=5e-4, batch_size=2000, rampup_epochs=2, sustain_epochs=0,
              exp_decay=0.8, weights_artifact="wandb_main_weights.h5", save_weights_only=True,
              checkpoint_metric="val_loss", save_freq="epoch", mode="min", save_best_weights=True, verbose=1,
              epochs=3, save_model=True, model_name="./wandb_anime_nn.h5",
              input_data="user_stats.parquet:latest", project_name="anime_recommendations",
              model_artifact="wandb_anime_nn.h5", history_csv="wandb_anime_nn_history.csv",
              ID_emb_name="user_embedding", anime_emb_name="anime_embedding", merged_name="dot_product",
              main_df_type="parquet", model_type="h5", history_type="history_csv", weights_type="h5",
              model_metrics='["mse"]', l2_reg_factor=1e-4)
    out = _run("neural_network", nn, str(work), env)
    return dict(work=work, env=env, paths=paths, nn_out=out)


def _common(pipeline):
    return dict(project_name="anime_recommendations", model="wandb_anime_nn.h5:latest", model_type="h5",
                main_df="user_stats.parquet:latest", main_df_type="parquet",
                anime_df="all_anime.csv:latest", anime_df_type="raw_data",
                ID_emb_name="user_embedding", anime_emb_name="anime_embedding")


def _model():
    from anime_recommendations_amd import artifacts, weights_io
    return weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest"))


@pytest.mark.parametrize("filters", [False, True])
def test_similar_anime_component_returns_300_rows(pipeline, filters):
    from anime_recommendations_amd import components as C, ops
    work, env = pipeline["work"], pipeline["env"]
    anime = pd.read_csv(pipeline["paths"]["all_anime"])
    query = anime["Name"].iloc[17]
    outs = {}
    for count in (300, 10):
        flags = dict(_common(pipeline), sypnopsis_df_type="raw_data", sypnopses_df="synopses.csv:latest",
                     anime_query=query, a_query_number=count, random_anime=False,
                     anime_rec_genres='[None, "Action", "Comedy"]', an_spec_genres=filters,
                     types='["TV", "Movie"]', spec_types=filters, a_rec_type="csv", save_sim_anime=True)
        _run("similar_anime", flags, str(work), env)
        outs[count] = pd.read_csv(work / (C.clean(query) + ".csv"))
    m = _model()
    ids = np.asarray(m["anime_ids"])
    q = int(np.nonzero(ids == anime["MAL_ID"].iloc[17])[0][0])
    meta = anime.set_index("MAL_ID").reindex(ids)
    keep = meta["Name"].notna().to_numpy()
    if filters:
        keep &= meta["Type"].isin(["TV", "Movie"]).to_numpy() & meta["Genres"].str.contains("Action|Comedy").to_numpy()
    s = ops.cosine_scores(ops.rownorm(torch.as_tensor(m["A"])), q).cpu().numpy()
    oi, os_ = orc.topk_desc(s, 300, exclude=q, mask=keep)
    out = outs[300]
    assert len(out) == min(300, len(oi)) and (filters or len(out) == 300)
    assert out["Name"].tolist() == meta["Name"].to_numpy()[oi].tolist()
    np.testing.assert_allclose(out["Similarity"].to_numpy(), os_, rtol=0, atol=1e-7)
    pd.testing.assert_frame_equal(outs[10], out.iloc[:10].reset_index(drop=True))


def test_similar_users_component_returns_every_neighbour(pipeline):
    from anime_recommendations_amd import components as C, ops
    work, env = pipeline["work"], pipeline["env"]
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    user = int(df.user_id.unique()[5])
    outs = {}
    for count in (500, 10):
        flags = dict(_common(pipeline), sim_user_query=user, id_query_number=count, max_ratings=600,
                     sim_random_user=False, num_faves=3, TV_only=True, sim_users_fn="similar_users.csv",
                     sim_users_type="csv", ID_fn="user_id.csv", ID_type="csv", save_sim_locally=True)
        _run("similar_users", flags, str(work), env)
        outs[count] = pd.read_csv(work / ("User_%d.csv" % user), keep_default_na=False)
    m = _model()
    ids = np.asarray(m["user_ids"])
    q = int(np.nonzero(ids == user)[0][0])
    s = ops.cosine_scores(ops.rownorm(torch.as_tensor(m["U"])), q).cpu().numpy()
    oi, os_ = orc.topk_desc(s, 500, exclude=q)
    out = outs[500]
    assert len(out) == len(ids) - 1 == len(oi)                 # min(count, the users a query can return)
    assert out["similar_users"].tolist() == ids[oi].tolist()
    np.testing.assert_allclose(out["similarity"].to_numpy(), os_, rtol=0, atol=1e-7)
    pd.testing.assert_frame_equal(outs[10], out.iloc[:10].reset_index(drop=True))


def test_model_recs_component_returns_every_unwatched_anime(pipeline):
    from anime_recommendations_amd import ops, weights_io
    work, env = pipeline["work"], pipeline["env"]
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    user = int(df.user_id.unique()[5])
    m = _model()
    ids = np.asarray(m["anime_ids"])
    outs = {}
    for count in (len(ids), 10):
        flags = dict(main_df="user_stats.parquet:latest", main_df_type="parquet", project_name="anime_recommendations",
                     anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopsis_df="synopses.csv:latest",
                     sypnopsis_df_type="raw_data", model="wandb_anime_nn.h5:latest", model_type="h5",
                     model_user_query=user, random_user=False, model_recs_fn="model_recs.csv", save_model_recs=True,
                     model_num_recs=count, anime_types='["TV", "Movie"]', specify_types=False,
                     model_genres='["Action", "Comedy", None]', specify_genres=False, model_ID_flow=True,
                     model_ID_conf=False, model_recs_type="csv", flow_ID="user_id.csv:latest", flow_ID_type="csv")
        _run("model_recs", flags, str(work), env)
        outs[count] = pd.read_csv(work / ("User_ID_%d_model_recs.csv" % user))
    uq = int(np.nonzero(np.asarray(m["user_ids"]) == user)[0][0])
    grid = ops.predict_grid(torch.as_tensor(m["U"]).cuda(), torch.as_tensor(m["A"]).cuda(),
                            weights_io.model_head(m), [uq])
    watched = set(df[df.user_id == user].anime_id)
    anime = pd.read_csv(pipeline["paths"]["all_anime"]).set_index("MAL_ID").reindex(ids)
    keep = ~np.isin(ids, list(watched)) & anime["Name"].notna().to_numpy()
    oi, op = orc.topk_desc(grid.cpu().numpy()[0], len(ids), mask=keep)
    out = outs[len(ids)]
    assert len(out) == int(keep.sum()) == len(oi)              # every unwatched anime: the user's full ranking
    assert out["anime_id"].tolist() == ids[oi].tolist()
    np.testing.assert_allclose(out["Prediction"].to_numpy(), op, rtol=0, atol=1e-7)
    pd.testing.assert_frame_equal(outs[10], out.iloc[:10].reset_index(drop=True))
