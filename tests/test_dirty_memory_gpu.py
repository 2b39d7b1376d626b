"""Every inference, ingest and favourites entry point on dirty memory (tests/poison.py).

Only the training ``workspace``, ``rowmap`` and ``lazy_state`` are documented "zero before first use"; every other
workspace, output array and flag word must give the same answer whatever bytes it held on entry.  Each case runs the
production wrapper once per pattern, with every ``torch.empty`` / ``torch.empty_like`` buffer filled with that byte:

 (a) every returned tensor is bit-identical to the 0x00 run (raw bits: NaN padding must match too);
 (b) what the call reports about its own work (fallback / re-run / flagged rows) is identical to the 0x00 run — a stale
     threshold that flags every row would otherwise hide behind the exact-path re-run;
 (c) the 0x00 run equals the oracle the suite already holds that call to, at that test's bar;
 (d) the 0x00 run is not degenerate (no fallback rows on random-normal tables, re-runs of the all-pairs job <= 2 %);
 and the poisoned bytes are at least the library's own workspace size plus the outputs, so that a refactor of the
 wrappers cannot turn a case into a no-op.

Further down: a job on the leftovers of a larger job in the cached workspace, every case a second time on the buffers
of its first run, and the count / flag words of the C ABI preset to 0x7F7F7F7F.
"""
import ctypes as C
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import poison
import prefs_restatement as R
from oracle import anirec_oracle as orc
from oracle import ingest_oracle, recs_oracle

pytestmark = pytest.mark.gpu

HEAD = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)      # the suite's head


class Case:
    """run(byte, log) -> (tensors, work); floor(tensors, work) -> bytes that must have been poisoned;
    check(tensors, work): (c) and (d) on the 0x00 run.  ``job``: the call goes through the cached job workspace."""

    def __init__(self, run, floor, check, job=False):
        self.run, self.floor, self.check, self.job = run, floor, check, job


def _bits(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t


def _same(got, want, tag):
    (gt, gw), (wt, ww) = got, want
    assert len(gt) == len(wt), tag
    for j, (g, w) in enumerate(zip(gt, wt)):
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, j)
        assert torch.equal(_bits(g), _bits(w)), (tag, "tensor %d differs" % j)
    assert gw == ww, (tag, "work done", gw, ww)


def _dirty(case, byte):
    from anime_recommendations_amd import ops
    log = []
    if case.job:
        ops.release_workspaces()            # the job workspace is cached: allocate it anew, through the patch
    with poison.poisoned(byte, log):
        res = case.run(byte, log)
    torch.cuda.synchronize()
    assert sum(log) >= case.floor(*res), (sum(log), case.floor(*res))
    return res


def _lib():
    from anime_recommendations_amd import _lib as L
    return L.load()


def _table(seed, n, zero=()):
    from anime_recommendations_amd import ops
    W = np.random.default_rng(seed).normal(0, 0.05, (n, 128)).astype(np.float32)
    for z in zero:
        W[z] = 0
    return ops.rownorm(torch.from_numpy(W))


# ---- oracles ---------------------------------------------------------------------------------------------------------
def _topk_oracle(scores, k, idx, val, exclude=None, mask=None, tag=None):
    """one row of a top-k result against orc.topk_desc over its score row: indices equal, scores equal (NaN == NaN),
    -1 / NaN padding behind the candidates"""
    oi, os_ = orc.topk_desc(scores, k, exclude=exclude, mask=mask)
    m = len(oi)
    assert (idx[:m] == oi).all(), tag
    assert np.array_equal(val[:m], os_, equal_nan=True), tag
    assert (idx[m:] == -1).all() and np.isnan(val[m:]).all(), tag
    return m


def _cosine_rows_oracle(Wh, queries, k, idx, val, rows=None, keep=None, exclude_self=True, tag=None):
    from anime_recommendations_amd import ops
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    queries = np.asarray(queries)
    short = 0
    for j in (range(len(queries)) if rows is None else rows):
        q = int(queries[j])
        s = ops.cosine_scores(Wh, q).cpu().numpy()
        m = _topk_oracle(s, k, idx[j], val[j], exclude=q if exclude_self else None,
                         mask=None if keep is None else np.asarray(keep, bool), tag=(tag, j))
        short += m < k
    return short


# ---- cosine_topk (exact kernels) -------------------------------------------------------------------------------------
def _exact_floor(n, nq, k, calls=1):
    lib = _lib()
    nb = lib.anirec_topk_large_workspace_bytes(n, nq, k) if k > 128 else lib.anirec_topk_workspace_bytes(n, nq)
    return calls * (int(nb) + 2 * nq * k * 4)


@functools.lru_cache(None)
def _case_topk_one_launch():
    """n 1000, 16 queries, k 10; row 9 is zero (NaN scores); keep leaves 7 candidates: padding over the poison"""
    from anime_recommendations_amd import ops
    n, k = 1000, 10
    Wh = _table(3, n, zero=(9,))
    keep = np.zeros(n, np.uint8)
    keep[:6] = 1
    keep[9] = 1
    q = np.array([2, 9, 300, 0, 999] + list(np.random.default_rng(4).integers(0, n, 11)), np.int32)

    def run(byte, log):
        return list(ops.cosine_topk(Wh, q, k, keep=keep) + ops.cosine_topk(Wh, q, k)), ()

    def check(t, work):
        assert _cosine_rows_oracle(Wh, q, k, t[0], t[1], keep=keep, tag="keep") == len(q)      # every row is padded
        assert _cosine_rows_oracle(Wh, q, k, t[2], t[3], tag="all") == 0
    return Case(run, lambda t, w: _exact_floor(n, len(q), k, 2), check)


@functools.lru_cache(None)
def _case_topk_sliced():
    """n 4608 >= 4096 and 3 queries < 1024: two slices of 2304 keys and the merge launch over the slice-winner lists;
    one keep mask empties the second slice, one leaves fewer than k candidates in the first alone"""
    from anime_recommendations_amd import ops
    n, k = 4608, 128
    Wh = _table(5, n)
    rng = np.random.default_rng(6)
    keep_a = (rng.random(n) > 0.3).astype(np.uint8)
    keep_a[2304:] = 0
    keep_b = np.zeros(n, np.uint8)
    keep_b[rng.choice(2304, 50, replace=False)] = 1
    q = np.array([7, 2304, 4607], np.int32)

    def run(byte, log):
        out = []
        for kp in (None, keep_a, keep_b):
            out += list(ops.cosine_topk(Wh, q, k, keep=kp))
        return out, ()

    def check(t, work):
        assert _cosine_rows_oracle(Wh, q, k, t[0], t[1], tag="all") == 0
        assert _cosine_rows_oracle(Wh, q, k, t[2], t[3], keep=keep_a, tag="slice emptied") == 0
        assert _cosine_rows_oracle(Wh, q, k, t[4], t[5], keep=keep_b, tag="few") == 3
    return Case(run, lambda t, w: _exact_floor(n, 3, k, 3), check)


@functools.lru_cache(None)
def _case_topk_query_batches():
    """16 queries on a workspace sized for 5 (poisoned by hand): the q0 += qb loop of anirec_cosine_topk"""
    from anime_recommendations_amd import ops
    n, k = 1000, 10
    Wh = _table(7, n, zero=(9,))
    q = np.array([9, 2, 999] + list(np.random.default_rng(8).integers(0, n, 13)), np.int32)
    nb = int(_lib().anirec_topk_workspace_bytes(n, 5))
    assert nb < int(_lib().anirec_topk_workspace_bytes(n, 16))
    held = {}

    def run(byte, log):
        if byte is None:                    # the second call of the same-call-twice test: the first call's workspace
            ws = held["ws"]
        else:
            ws = held["ws"] = torch.empty(nb, dtype=torch.uint8, device="cuda")
            poison.fill(ws, byte)
        return list(ops.cosine_topk(Wh, q, k, workspace=ws)), ()

    def check(t, work):
        assert _cosine_rows_oracle(Wh, q, k, t[0], t[1], tag="batches") == 0
    return Case(run, lambda t, w: nb + 2 * len(q) * k * 4, check)


@functools.lru_cache(None)
def _case_topk_large_k():
    """k 300 of n 1000: the one-workgroup LDS sort; k = n = 21 000 (above its 20 480 limit): tiles + merge passes"""
    from anime_recommendations_amd import ops
    Wa, Wb = _table(9, 1000, zero=(17,)), _table(10, 21_000, zero=(17,))
    keep_a = (np.random.default_rng(11).random(1000) > 0.8).astype(np.uint8)          # ~200 candidates: padding
    keep_b = (np.random.default_rng(12).random(21_000) > 0.1).astype(np.uint8)
    qa, qb = np.array([17, 3, 999, 500], np.int32), np.array([17, 20_999], np.int32)

    def run(byte, log):
        out = list(ops.cosine_topk(Wa, qa, 300)) + list(ops.cosine_topk(Wa, qa, 300, keep=keep_a))
        out += list(ops.cosine_topk(Wb, qb, 21_000, keep=keep_b))
        return out, ()

    def check(t, work):
        assert _cosine_rows_oracle(Wa, qa, 300, t[0], t[1], tag="lds") == 0
        assert _cosine_rows_oracle(Wa, qa, 300, t[2], t[3], keep=keep_a, tag="lds keep") == 4
        assert _cosine_rows_oracle(Wb, qb, 21_000, t[4], t[5], keep=keep_b, tag="tiles") == 2
    return Case(run, lambda t, w: _exact_floor(1000, 4, 300, 2) + _exact_floor(21_000, 2, 21_000), check)


# ---- cosine_topk_mfma ------------------------------------------------------------------------------------------------
def _mfma(Wh, q, k, **kw):
    """one job -> (tensors, work done, stats)"""
    from anime_recommendations_amd import ops
    stats = {}
    idx, sim, n_fb = ops.cosine_topk_mfma(Wh, q, k, stats=stats, **kw)
    fr = stats.get("flag_rows")
    work = (n_fb, stats["rerun_rows"], stats["fallback_rows"], None if fr is None else tuple(sorted(fr.items())))
    return [idx, sim], work, stats


def _mfma_floor(n, nq, k, stats):
    lib = _lib()
    rows = int(np.diff(stats["starts"]).max())
    fn = lib.anirec_cosine_topk_allpairs_workspace_bytes if stats["allpairs"] else lib.anirec_cosine_topk_job_workspace_bytes
    return int(fn(n, rows, stats["lanes"])) + 2 * nq * k * 4 + nq * 4


class MfmaCase(Case):
    """variants: name -> (Wh, queries, k, kwargs, env, expectation); run as one job each, in order"""

    def __init__(self, variants, probe, plan=None):
        self.variants, self.probe, self.plan, self.job, self.stats = variants, probe, plan, True, {}

    def run(self, byte, log):
        from anime_recommendations_amd import ops
        tensors, work = [], []
        for name, (Wh, q, k, kw, env, _) in self.variants.items():
            old = {e: os.environ.get(e) for e in env}
            os.environ.update(env)
            try:
                if byte is not None and tensors:
                    ops.release_workspaces()        # each job of the case on a workspace of its own, poisoned
                t, w, st = _mfma(Wh, q, k, **kw)
            finally:
                for e, v in old.items():
                    os.environ.pop(e) if v is None else os.environ.__setitem__(e, v)
            tensors += t
            work.append(w)
            self.stats[name] = st
        return tensors, tuple(work)

    def floor(self, tensors, work):
        return sum(_mfma_floor(Wh.shape[0], len(q), k, self.stats[name])
                   for name, (Wh, q, k, _, _, _) in self.variants.items())

    def check(self, tensors, work):
        for j, (name, (Wh, q, k, kw, env, expect)) in enumerate(self.variants.items()):
            n_fb, rerun, fb_rows, flag_rows = work[j]
            nq = len(q)
            assert fb_rows == 0 and n_fb == 0, (name, work[j])                       # (d): random-normal rows
            if expect == "all rerun":
                assert rerun == nq, (name, rerun)
            elif expect == "allpairs":
                assert self.stats[name]["allpairs"] is True and rerun <= 0.02 * nq, (name, rerun)
            elif expect == "no prior":
                assert rerun == 0 and flag_rows is None, (name, work[j])
            self.probe(name, Wh, q, k, tensors[2 * j], tensors[2 * j + 1], self.stats[name])
        if self.plan:
            self.plan(self.stats)


def _probe_rows(rows):
    def probe(name, Wh, q, k, idx, sim, stats):
        qn = q.cpu().numpy() if torch.is_tensor(q) else np.asarray(q)
        _cosine_rows_oracle(Wh, qn, k, idx, sim, rows=rows(len(qn)), tag=name)
    return probe


@functools.lru_cache(None)
def _case_mfma_one_batch():
    """n = nq = 1000, k 10, no prior; 333 x 333 at k 127: a ragged last key tile, k_eff + 16 next to kKept"""
    rng = np.random.default_rng(13)
    Wa, Wb = _table(14, 1000), _table(15, 333)
    v = {"1000": (Wa, rng.permutation(1000).astype(np.int32), 10, dict(prior=None), {}, "no prior"),
         "333": (Wb, rng.permutation(333).astype(np.int32), 127, dict(prior=None), {}, "no prior")}
    return MfmaCase(v, _probe_rows(lambda nq: range(nq)))


@functools.lru_cache(None)
def _case_mfma_lanes():
    """n 2000, the queries a permutation, k 30, batches of 256 on 1, 2 and 4 chains; an explicit prior (mode 2), and
    one above every cosine (every row unproven and re-run: the same count every time)"""
    n = 2000
    Wh = _table(16, n)
    q = np.random.default_rng(17).permutation(n).astype(np.int32)
    v = {"lanes%d" % ln: (Wh, q, 30, dict(batch=256, prior=None, lanes=ln), {}, "no prior") for ln in (1, 2, 4)}
    v["prior0.2"] = (Wh, q, 30, dict(batch=256, prior=0.2, lanes=2), {}, None)
    v["prior0.999"] = (Wh, q, 30, dict(batch=256, prior=0.999, lanes=2), {}, "all rerun")
    return MfmaCase(v, _probe_rows(lambda nq: range(0, nq, 7)))


@functools.lru_cache(None)
def _case_mfma_splits():
    """18 000 keys, 3 000 queries, k 10: the key tiles of a super-step on 1 and on 4 workgroups per row block"""
    Wh = _table(5, 18_000)
    q = torch.arange(3_000, dtype=torch.int32, device="cuda")
    v = {"splits%s" % sp: (Wh, q, 10, {}, {"ANIREC_TOPK_SPLITS": sp}, "no prior") for sp in ("1", "4")}
    return MfmaCase(v, _probe_rows(lambda nq: range(0, nq, 12)))


N_BIG = 49_152          # where the default plan starts to learn a prior from its first batch ...
K_BIG = 32              # ... if k >= 32 (anirec_cosine_topk_job_plan: below that a prior buys nothing and none is learnt)


@functools.lru_cache(None)
def _big_table():
    from anime_recommendations_amd import ops
    g = torch.Generator(device="cuda")
    g.manual_seed(21)
    Wh = ops.rownorm(torch.randn(N_BIG, 128, generator=g, device="cuda") * 0.05)
    return Wh, torch.arange(N_BIG, dtype=torch.int32, device="cuda")


@functools.lru_cache(None)
def _big_oracle():
    """the oracle lists (k = K_BIG; a smaller k is their prefix) of ~500 probe rows of the 49 152-row table, around every
    batch start of both plans: computed once, shared by the learnt-prior and the all-pairs cases"""
    from anime_recommendations_amd import ops
    Wh, _ = _big_table()
    edges = [0, 16384, 32768, N_BIG]
    rows = np.unique(np.concatenate([np.arange(max(e - 40, 0), min(e + 40, N_BIG)) for e in edges] +
                                    [np.arange(0, N_BIG, 200)]))
    out = {}
    for r in rows:
        out[int(r)] = orc.topk_desc(ops.cosine_scores(Wh, int(r)).cpu().numpy(), K_BIG, exclude=int(r))
    return out


def _big_probe(name, Wh, q, k, idx, sim, stats):
    want = _big_oracle()
    assert k <= K_BIG
    assert all(s_ in want for s_ in stats["starts"][:-1]) and len(want) >= 450
    rows = torch.tensor(sorted(want), device="cuda")
    gi, gs = idx[rows].cpu().numpy(), sim[rows].cpu().numpy()
    for j, r in enumerate(sorted(want)):
        assert (gi[j] == want[r][0][:k]).all() and (gs[j] == want[r][1][:k]).all(), (name, r)


@functools.lru_cache(None)
def _case_mfma_learnt_prior():
    """n = nq = 49 152, k 32: a first batch of 16 384 rows without a prior, the others under the one it gives.  At k 10
    the plan learns none: one plain batch, on the 256-row workgroups that 49 152 queries select."""
    Wh, q = _big_table()
    def plan(stats):
        st = stats["learnt"]
        assert st["learn_batches"] == 1 and st["starts"] == [0, 16384, N_BIG] and st["allpairs"] is False
        assert stats["k10"]["learn_batches"] == 0 and stats["k10"]["batches"] == 1
    return MfmaCase({"k10": (Wh, q, 10, dict(allpairs=False), {}, "no prior"),
                     "learnt": (Wh, q, K_BIG, dict(allpairs=False), {}, None)}, _big_probe, plan)


@functools.lru_cache(None)
def _case_mfma_allpairs():
    """the same table as an all-pairs job (prior_mode 3) on 1 and 2 chains: inboxes, their counters, the waves' logs
    and the overflow word of the misc block are all in play"""
    Wh, q = _big_table()
    v = {"lanes%d" % ln: (Wh, q, K_BIG, dict(batch=16384, allpairs=True, lanes=ln), {}, "allpairs") for ln in (1, 2)}
    return MfmaCase(v, _big_probe)


# ---- predict ---------------------------------------------------------------------------------------------------------
def _watched(rng, nq, n_a, frac):
    w = rng.random((nq, n_a)) < frac
    return w, R.pack(w).view(np.int32)


@functools.lru_cache(None)
def _case_predict_grid():
    """257 users x 1001 anime (the dword-store MFMA kernel), 40 x 4160 (n_anime % 4 == 0: the row-quad kernel); one
    zero user row"""
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(22)
    U = rng.normal(0, 0.05, (300, 128)).astype(np.float32)
    U[7] = 0
    shapes = []
    for nq, n_a in ((257, 1001), (40, 4160)):
        A = rng.normal(0, 0.05, (n_a, 128)).astype(np.float32)
        users = np.concatenate([[7, 0, 299], rng.integers(0, 300, nq - 3)]).astype(np.int32)
        shapes.append((A, torch.from_numpy(A).cuda(), users))
    tU = torch.from_numpy(U).cuda()

    def run(byte, log):
        out = []
        for _, tA, users in shapes:
            out += [ops.predict_grid(tU, tA, HEAD, users), ops.predict_grid_mfma(tU, tA, HEAD, users)]
        return out, ()

    def floor(t, w):
        lib = _lib()
        return sum(int(lib.anirec_predict_workspace_bytes(A.shape[0], len(us), 0)) +
                   int(lib.anirec_predict_mfma_workspace_bytes(A.shape[0], len(us))) + 2 * len(us) * A.shape[0] * 4
                   for A, _, us in shapes)

    def check(t, work):
        for j, (A, _, users) in enumerate(shapes):
            want = orc.predict_grid(U, A, orc.new_head(**HEAD), users)
            np.testing.assert_allclose(t[2 * j].cpu().numpy(), want, atol=1e-5)
            np.testing.assert_allclose(t[2 * j + 1].cpu().numpy(), want, atol=1e-5)
    return Case(run, floor, check)


def _predict_rows_oracle(tU, tA, head, users, k, watched, idx, p, tag):
    """rows of a predict top-k against orc.topk_desc over the fp32 rating grid; returns the number of padded rows"""
    from anime_recommendations_amd import ops
    G = ops.predict_grid(tU, tA, head, users).cpu().numpy()
    idx, p = idx.cpu().numpy(), p.cpu().numpy()
    short = 0
    for j in range(len(users)):
        short += _topk_oracle(G[j], k, idx[j], p[j], mask=None if watched is None else ~watched[j], tag=(tag, j)) < k
    return short


@functools.lru_cache(None)
def _case_predict_topk():
    """5 users x 1234 anime, k 10, 30 % watched, one user with 4 unwatched anime; 3 x 4608 (the sliced select with the
    watched bits); k 1300 on the first table (the large path)"""
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(23)
    tU = torch.from_numpy(rng.normal(0, 0.05, (50, 128)).astype(np.float32)).cuda()
    tA = torch.from_numpy(rng.normal(0, 0.05, (1234, 128)).astype(np.float32)).cuda()
    tB = torch.from_numpy(rng.normal(0, 0.05, (4608, 128)).astype(np.float32)).cuda()
    ua, ub = np.array([5, 0, 49, 12, 33], np.int32), np.array([1, 48, 20], np.int32)
    wa, _ = _watched(rng, 5, 1234, 0.3)
    wa[3] = True
    wa[3, [0, 617, 1200, 1233]] = False
    ba = R.pack(wa).view(np.int32)
    wb, bb = _watched(rng, 3, 4608, 0.3)
    runs = [(tA, ua, 10, wa, ba), (tB, ub, 10, wb, bb), (tB, ub, 128, None, None), (tA, ua, 1300, wa, ba)]

    def run(byte, log):
        out = []
        for A, us, k, _, bits in runs:
            out += list(ops.predict_topk(tU, A, HEAD, us, k, bits))
        return out, ()

    def floor(t, w):
        lib = _lib()
        return sum(int(lib.anirec_predict_topk_large_workspace_bytes(A.shape[0], len(us), k) if k > 128
                       else lib.anirec_predict_workspace_bytes(A.shape[0], len(us), 1)) + 2 * len(us) * k * 4
                   for A, us, k, _, _ in runs)

    def check(t, work):
        short = [_predict_rows_oracle(tU, A, HEAD, us, k, w, t[2 * j], t[2 * j + 1], j)
                 for j, (A, us, k, w, _) in enumerate(runs)]
        assert short == [1, 0, 0, 5], short         # k 1300 of ~860 unwatched: every row padded
    return Case(run, floor, check)


@functools.lru_cache(None)
def _case_predict_topk_mfma():
    """300 users x 1001 anime, k 10, with and without the watched mask, a rising and a falling head; one user with
    fewer than k unwatched anime: flagged the same way every time; and in batches of 128 users (128, 128, 44) on one
    workspace and one flags array, as the wrapper cuts a large user list"""
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(24)
    n_q, n_a, k = 300, 1001, 10
    tU = torch.from_numpy(rng.normal(0, 0.05, (400, 128)).astype(np.float32)).cuda()
    tA = torch.from_numpy(rng.normal(0, 0.05, (n_a, 128)).astype(np.float32)).cuda()
    users = rng.permutation(400)[:n_q].astype(np.int32)
    w = rng.random((n_q, n_a)) < 0.3
    w[11] = True
    w[11, [3, 500, 1000]] = False
    bits = R.pack(w).view(np.int32)
    heads = [dict(HEAD, w=1.7), dict(HEAD, w=-1.7)]
    runs = [(h, wm, bm) for h in heads for wm, bm in ((None, None), (w, bits))]

    def run(byte, log):
        out, work = [], []
        for h, _, bm in runs:
            i1, p1, f1 = ops.predict_topk_mfma(tU, tA, h, users, k, bm)
            i2, p2, f2 = ops.predict_topk_mfma(tU, tA, h, users, k, bm, fallback=False)
            i3, p3, f3 = ops.predict_topk_mfma(tU, tA, h, users, k, bm, batch=128)
            out += [i1, p1, i2, p2, i3, p3]
            work.append((f1, f2, f3))
        return out, tuple(work)

    def floor(t, wk):
        lib = _lib()
        whole = int(lib.anirec_predict_topk_mfma_workspace_bytes(n_a, n_q)) + 2 * n_q * k * 4 + n_q * 4
        cut = int(lib.anirec_predict_topk_mfma_workspace_bytes(n_a, 128)) + 2 * n_q * k * 4 + 128 * 4
        return len(runs) * (2 * whole + cut)

    def check(t, work):
        for j, (h, wm, _) in enumerate(runs):
            f1, f2, f3 = work[j]
            i1, p1, i2, _, i3, p3 = t[6 * j:6 * j + 6]
            short = _predict_rows_oracle(tU, tA, h, users, k, wm, i1, p1, j)
            assert short == (0 if wm is None else 1)
            # the bars of test_predict_topk_mfma_equals_exact_path_bitwise; the short row must be among the flagged
            assert f1 == f2 == f3 and (f1 <= 2 if wm is None else 1 <= f1 <= 4), (j, work[j])
            assert torch.equal(i3, i1) and torch.equal(_bits(p3), _bits(p1)), j
            i2 = i2.cpu().numpy()
            ok = i2[:, 0] >= 0                       # without the fallback a flagged row is -1 / NaN, never wrong
            assert (i2[ok] == i1.cpu().numpy()[ok]).all() and (~ok).sum() <= f2
    return Case(run, floor, check)


# ---- ingest ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _case_preprocess():
    """16 385 rows: one row past a 8 192-row chunk pair, so the keep flags and tile sums of the padding rows matter;
    shuffled and grouped by user, drop_half_watched on and off, with nulls; 5 000 rows of which nothing survives"""
    from anime_recommendations_amd import ingest
    from test_ingest_gpu import _raw_frame
    frames = []
    for grouped in (False, True):
        df = _raw_frame(16_385, 300, 700, seed=31, grouped=grouped)
        for dhw in (False, True):
            frames.append((df, ingest.frame_to_columns(df), 30, dhw))
    df = _raw_frame(5_000, 200, 100, seed=7)
    frames.append((df, ingest.frame_to_columns(df), 10 ** 6, False))
    names = ("user_id", "anime_id", "rating", "watching_status", "watched_episodes", "max_eps", "half_eps")

    def run(byte, log):
        out = []
        for _, cols, nr, dhw in frames:
            got = ingest.preprocess_columns(cols, nr, drop_half_watched=dhw)
            out += [got[c] for c in names if c in got]
        return out, ()

    def floor(t, w):
        return sum(int(_lib().anirec_ingest_workspace_bytes(len(df), cols.bounds["user_id"], cols.bounds["anime_id"])) +
                   len(df) * (4 * 4 + 8 + (12 if dhw else 0)) for df, cols, _, dhw in frames)

    def check(t, work):
        at = 0
        for df, _, nr, dhw in frames:
            want = ingest_oracle.preprocess(df, nr, False, False, dhw)
            cols = [c for c in names if dhw or c not in ("max_eps", "half_eps")]
            got = dict(zip(cols, t[at:at + len(cols)]))
            at += len(cols)
            assert len(got["user_id"]) == len(want) and (nr > 1000 or 0 < len(want) < len(df))
            for c in ("user_id", "anime_id", "watching_status", "watched_episodes"):
                np.testing.assert_array_equal(got[c].cpu().numpy().astype(np.int64), want[c].to_numpy().astype(np.int64), c)
            np.testing.assert_array_equal(got["rating"].cpu().numpy().view(np.uint64),
                                          want["rating"].to_numpy().astype(np.float64).view(np.uint64))
            if dhw:
                np.testing.assert_array_equal(got["max_eps"].cpu().numpy(), want["max_eps"].to_numpy().astype(np.int64))
                np.testing.assert_array_equal(got["half_eps"].cpu().numpy(), want["half_eps"].to_numpy().astype(np.float64))
    return Case(run, floor, check)


@functools.lru_cache(None)
def _case_encode():
    """200 003 ids below 32 768 (the id tables in LDS) and below 32 769 (the global table); a single id"""
    from anime_recommendations_amd import ingest
    rng = np.random.default_rng(32)
    cols = []
    for n, bound in ((200_003, 32_768), (200_003, 32_769), (1, 10)):
        ids = rng.integers(0, bound, n).astype(np.int32)
        ids[-1] = bound - 1
        cols.append((ids, torch.as_tensor(ids, device="cuda"), bound))

    def run(byte, log):
        out = []
        for _, t, bound in cols:
            out += list(ingest.encode_ids(t, bound=bound))
        return out, ()

    def floor(t, w):
        return sum(int(_lib().anirec_ingest_encode_workspace_bytes(len(ids), b)) + 4 * len(ids) + 4 * min(len(ids), b)
                   for ids, _, b in cols)

    def check(t, work):
        for j, (ids, _, _) in enumerate(cols):
            want_idx, want_uniq = ingest_oracle.encode(pd.Series(ids))
            np.testing.assert_array_equal(t[2 * j].cpu().numpy(), want_idx)
            np.testing.assert_array_equal(t[2 * j + 1].cpu().numpy(), want_uniq)
    return Case(run, floor, check)


# ---- favourites and recommendations ----------------------------------------------------------------------------------
@functools.lru_cache(None)
def _case_favourites():
    """301 users x 33 anime: 602 bit words, not a multiple of 4 (the memset branch); 300 x 1024 (k_rec_clear); grouped
    by user and shuffled; 20 users without a rating; the 80th percentile"""
    from anime_recommendations_amd import recs
    tables = []
    for n_users, n_anime in ((301, 33), (300, 1024)):
        rng = np.random.default_rng(n_users)
        sizes = rng.integers(1, min(n_anime, 40) + 1, n_users)
        sizes[rng.choice(n_users, 20, replace=False)] = 0
        u = np.repeat(np.arange(n_users), sizes).astype(np.int32)
        a = np.concatenate([rng.choice(n_anime, s, replace=False) for s in sizes]).astype(np.int32)
        r = (rng.integers(0, 11, len(u)) / 10).astype(np.float64)
        for grouped in (True, False):
            p = np.arange(len(u)) if grouped else rng.permutation(len(u))
            tables.append((u[p], a[p], r[p], n_users, n_anime))

    def run(byte, log):
        out = []
        for u, a, r, n_users, n_anime in tables:
            out += list(recs.user_favourites(torch.as_tensor(u).cuda(), torch.as_tensor(a).cuda(),
                                             torch.as_tensor(r).cuda(), n_users, n_anime, 80.0))
        return out, ()

    def floor(t, w):
        return sum(int(_lib().anirec_fav_workspace_bytes(len(u), nu)) + nu * ((na + 31) // 32) * 4 + nu * 8
                   for u, _, _, nu, na in tables)

    def check(t, work):
        for j, (u, a, r, n_users, n_anime) in enumerate(tables):
            thr_o, fav_o = recs_oracle.favourites(u, a, r, n_users, 80)
            thr = t[2 * j + 1].cpu().numpy()
            ok = ~np.isnan(thr_o)
            assert (~ok).sum() == 20 and np.array_equal(np.isnan(thr), ~ok)
            assert np.array_equal(thr[ok].view(np.uint64), thr_o[ok].view(np.uint64))
            want = np.zeros((n_users, n_anime), bool)
            for uu in range(n_users):
                want[uu, sorted(fav_o[uu])] = True
            np.testing.assert_array_equal(t[2 * j].cpu().numpy().view(np.uint32), R.pack(want))
    return Case(run, floor, check)


@functools.lru_cache(None)
def _case_recs():
    """user_recs, user_recs_ex and fave_profile at the smallest rows of the existing sweeps: (k_sim, n_recs) = (1, 7)
    and (63, 256) at 31 anime — fewer hits than n_recs: -1 / 0 padding over the poison; 33 categories at 33 anime"""
    from anime_recommendations_amd import recs
    rng = np.random.default_rng(33)
    n_users, nq = 90, 40
    fav31, fav33 = R.pack(rng.random((n_users, 31)) < 0.3), R.pack(rng.random((n_users, 33)) < 0.3)
    fav31[4] = 0
    t31, t33 = torch.from_numpy(fav31.view(np.int32)).cuda(), torch.from_numpy(fav33.view(np.int32)).cuda()
    queries = rng.integers(0, n_users, nq).astype(np.int32)
    sims = {ks: rng.integers(0, n_users, (nq, ks)).astype(np.int32) for ks in (1, 63)}
    sims[63][1, 30:] = -1
    sims[1][2, 0] = -1
    excl, keep = R.pack(rng.random((nq, 31)) < 0.1), R.pack(rng.random(31) < 0.7)
    cat = R.pack(rng.random((33, 33)) < 0.2)
    prof_users = [3, 0, 4, 3, 89, 17]
    sweeps = ((1, 7), (63, 256))

    def run(byte, log):
        out = []
        for ks, nr in sweeps:
            out += list(recs.user_recs(t31, 31, queries, sims[ks], nr))
            out += list(recs.user_recs(t31, 31, None, sims[ks], nr, exclude=excl, keep=keep))
        out += [recs.fave_profile(t33, cat, 33), recs.fave_profile(t33, cat, 33, users=prof_users)]
        return out, ()

    def floor(t, w):
        return sum(2 * 2 * nq * nr * 4 for _, nr in sweeps) + (n_users + len(prof_users)) * 33 * 4

    def check(t, work):
        favs = [set(np.nonzero(r)[0].tolist()) for r in R.unpack(fav31, 31)]
        ks_ = set(np.nonzero(R.unpack(keep, 31))[0].tolist())
        padded = 0
        for j, (ks, nr) in enumerate(sweeps):
            a0, c0, a1, c1 = (x.cpu().numpy() for x in t[4 * j:4 * j + 4])
            for i in range(nq):
                wa, wc = recs_oracle.user_recs(favs, int(queries[i]), sims[ks][i].tolist(), nr)
                ex = set(np.nonzero(R.unpack(excl[i], 31))[0].tolist())
                xa, xc = R.user_recs(favs, ex, sims[ks][i].tolist(), nr, ks_)
                for ga, gc, oa, oc in ((a0[i], c0[i], wa, wc), (a1[i], c1[i], xa, xc)):
                    m = len(oa)
                    assert ga[:m].tolist() == list(oa) and gc[:m].tolist() == list(oc), (ks, nr, i)
                    assert (ga[m:] == -1).all() and (gc[m:] == 0).all(), (ks, nr, i)
                    padded += m < nr
        assert padded > 2 * nq                       # 31 anime < 256: every row of that sweep, and some of (1, 7)
        np.testing.assert_array_equal(t[8].cpu().numpy(), R.fave_profile(fav33, 33, cat, 33))
        np.testing.assert_array_equal(t[9].cpu().numpy(), R.fave_profile(fav33, 33, cat, 33, users=prof_users))
    return Case(run, floor, check)


@functools.lru_cache(None)
def _case_plain_outputs():
    """the calls without a workspace, whose output is their only buffer: rownorm (a zero row: NaN), cosine_scores,
    predict_pairs, gather_ratings — sizes that end inside a workgroup"""
    from anime_recommendations_amd import ops
    rng = np.random.default_rng(35)
    n, m = 1001, 3001
    W = rng.normal(0, 0.05, (n, 128)).astype(np.float32)
    W[17] = 0
    tW = torch.from_numpy(W).cuda()
    Wh = ops.rownorm(tW)
    U = rng.normal(0, 0.05, (300, 128)).astype(np.float32)
    tU = torch.from_numpy(U).cuda()
    ui, ai = rng.integers(0, 300, m), rng.integers(0, n, m)
    r = rng.random(m).astype(np.float32)
    perm = rng.permutation(m)
    tui, tai, tr = (torch.as_tensor(x).cuda() for x in (ui.astype(np.int32), ai.astype(np.int32), r))

    def run(byte, log):
        return [ops.rownorm(tW), ops.cosine_scores(Wh, 5), ops.predict_pairs(tU, tW, HEAD, ui, ai),
                *ops.gather_ratings(tui, tai, tr, perm)], ()

    def check(t, work):
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = orc.rownorm(W)
        got = t[0].cpu().numpy()
        ok = ~np.isnan(ref)
        assert np.isnan(got[17]).all() and not ok[17].any()
        np.testing.assert_allclose(got[ok], ref[ok], rtol=3e-7, atol=0)
        Whn = Wh.cpu().numpy()
        keep = np.arange(n) != 17
        np.testing.assert_allclose(t[1].cpu().numpy()[keep], orc.dot_chain_f32(Whn, Whn[5])[keep], atol=1.2e-7)
        np.testing.assert_allclose(t[2].cpu().numpy(), orc.predict_pairs(U, W, orc.new_head(**HEAD), ui, ai), atol=1e-5)
        for got, src in zip(t[3:], (ui, ai, r)):
            np.testing.assert_array_equal(got.cpu().numpy(), src[perm])
    return Case(run, lambda t, w: n * 512 + n * 4 + m * 4 + m * 12, check)


CASES = {
    "plain_outputs": _case_plain_outputs,
    "cosine_topk-one_launch": _case_topk_one_launch,
    "cosine_topk-sliced_select": _case_topk_sliced,
    "cosine_topk-query_batches": _case_topk_query_batches,
    "cosine_topk-large_k": _case_topk_large_k,
    "cosine_topk_mfma-one_batch": _case_mfma_one_batch,
    "cosine_topk_mfma-lanes_and_batches": _case_mfma_lanes,
    "cosine_topk_mfma-key_range_splits": _case_mfma_splits,
    "cosine_topk_mfma-learnt_prior": _case_mfma_learnt_prior,
    "cosine_topk_mfma-allpairs": _case_mfma_allpairs,
    "predict_grid": _case_predict_grid,
    "predict_topk": _case_predict_topk,
    "predict_topk_mfma": _case_predict_topk_mfma,
    "ingest-preprocess_columns": _case_preprocess,
    "ingest-encode_ids": _case_encode,
    "recs-user_favourites": _case_favourites,
    "recs-user_recs_and_profiles": _case_recs,
}
_BASE = {}


def _baseline(name):
    """the 0x00 run of a case, checked against its oracle the first time it is needed"""
    if name not in _BASE:
        case = CASES[name]()
        res = _dirty(case, 0x00)
        case.check(*res)
        _BASE[name] = res
    return _BASE[name]


@pytest.mark.parametrize("byte", poison.ORDER, ids=["0x%02X" % b for b in poison.ORDER])
@pytest.mark.parametrize("name", list(CASES))
def test_results_do_not_depend_on_what_the_buffers_held(name, byte):
    base = _baseline(name)                           # (c), (d) and the poisoned-bytes floor of the 0x00 run
    if byte != 0x00:
        _same(_dirty(CASES[name](), byte), base, (name, "0x%02X" % byte))       # (a), (b) and the floor


@pytest.mark.parametrize("name", list(CASES))
def test_same_call_twice_on_the_buffers_of_its_first_run(name):
    """Nothing patched: the second call gets what the first left behind — the same ``workspace=`` where the wrapper
    takes one, the cached job workspace, otherwise the allocator's reuse of the blocks just freed."""
    case = CASES[name]()
    base = _baseline(name)
    first = case.run(0x00, [])
    second = case.run(None, [])
    torch.cuda.synchronize()
    _same(first, base, (name, "first"))
    _same(second, base, (name, "second"))


def test_a_job_on_the_leftovers_of_a_larger_job():
    """One cached workspace, as similar_users followed by similar_anime leave it in one process: the all-pairs job, the
    1000 x 1000 one-batch job, the 2000-row job on four chains and the all-pairs job again on one chain.  Each equals
    the same call on a workspace of its own."""
    from anime_recommendations_amd import ops
    big, one, lanes = _case_mfma_allpairs().variants, _case_mfma_one_batch().variants, _case_mfma_lanes().variants
    seq = [big["lanes2"], one["1000"], lanes["lanes4"], big["lanes1"]]
    own = []
    for Wh, q, k, kw, _, _ in seq:
        ops.release_workspaces()
        own.append(_mfma(Wh, q, k, **kw)[:2])
    ops.release_workspaces()
    held = None
    for j, (Wh, q, k, kw, _, _) in enumerate(seq):
        got = _mfma(Wh, q, k, **kw)[:2]
        ws = next(iter(ops._JOB_WS.values()))
        held = ws if held is None else held
        assert ws is held, "job %d did not run on the first job's buffer" % j
        _same(got, own[j], ("leftovers", j))
    ops.release_workspaces()


# ---- the count and flag words of the C ABI ---------------------------------------------------------------------------
FULL = 0x7F7F7F7F


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dirty_ws(nbytes):
    return poison.fill(torch.empty(int(nbytes), dtype=torch.uint8, device="cuda"), 0x7F)


def _words():
    """[count int64 | flag int32 in an int64 slot], every byte 0x7F"""
    res = poison.fill(torch.empty(2, dtype=torch.int64, device="cuda"), 0x7F)
    assert res.view(torch.int32).tolist() == [FULL] * 4
    return res, res[0:1], res[1:2].view(torch.int32)[0:1]


def test_ingest_calls_overwrite_their_count_and_flag_words():
    """include/anirec.h says "becomes 1 if": a ctypes caller need not clear n_out, n_unique, out_max2 or err_flag"""
    from anime_recommendations_amd import _lib as L, ingest
    from test_ingest_gpu import _raw_frame
    lib = L.load()
    df = _raw_frame(16_385, 300, 700, seed=31, nulls=False)
    cols = ingest.frame_to_columns(df)
    n = len(df)
    u, a, r, s, e = (cols[c] for c in ingest.COLUMNS)
    # id_max
    mx = poison.fill(torch.empty(2, dtype=torch.int32, device="cuda"), 0x7F)
    L.check(lib.anirec_ingest_id_max(L.ptr(u), L.ptr(a), n, L.ptr(mx), _stream()))
    assert mx.tolist() == [int(df.user_id.max()), int(df.anime_id.max())]
    ub, ab = mx[0].item() + 1, mx[1].item() + 1
    want = ingest_oracle.preprocess(df, 30)
    for bad_row in (None, 5):
        uu = u.clone()
        if bad_row is not None:
            uu[bad_row] = ub                         # one id outside its bound
        opts = L.IngestOpts(30, 0, 0, 0, ub, ab)
        out = [poison.fill(torch.empty_like(x), 0x7F) for x in (u, a, r, s, e)]
        res, n_out, err = _words()
        ws = _dirty_ws(lib.anirec_ingest_workspace_bytes(n, ub, ab))
        L.check(lib.anirec_ingest_preprocess(L.ptr(uu), L.ptr(a), L.ptr(r), L.ptr(s), L.ptr(e), n, C.byref(opts),
                                             *[L.ptr(x) for x in out], L.ptr(n_out), L.ptr(err), L.ptr(ws), ws.numel(),
                                             _stream()))
        m, flag = res.view(torch.int32)[0:3:2].tolist()
        assert res.view(torch.int32)[1].item() == 0              # the upper half of the 64-bit count too
        if bad_row is None:
            assert m == len(want) and flag == 0
            np.testing.assert_array_equal(out[0][:m].cpu().numpy(), want["user_id"].to_numpy())
        else:
            assert flag == 1
    # encode
    ids = cols["anime_id"]
    want_idx, want_uniq = ingest_oracle.encode(pd.Series(ids.cpu().numpy()))
    for bad_row in (None, 5):
        ii = ids.clone()
        if bad_row is not None:
            ii[bad_row] = -3
        idx, uniq = poison.fill(torch.empty_like(ids), 0x7F), poison.fill(torch.empty_like(ids), 0x7F)
        res, n_u, err = _words()
        ws = _dirty_ws(lib.anirec_ingest_encode_workspace_bytes(n, ab))
        L.check(lib.anirec_ingest_encode(L.ptr(ii), n, ab, L.ptr(idx), L.ptr(uniq), L.ptr(n_u), L.ptr(err), L.ptr(ws),
                                         ws.numel(), _stream()))
        cnt, flag = res[0].item(), res.view(torch.int32)[2].item()
        if bad_row is None:
            assert cnt == len(want_uniq) and flag == 0
            np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
            np.testing.assert_array_equal(uniq[:cnt].cpu().numpy(), want_uniq)
        else:
            assert flag == 1


def test_favourites_and_profile_calls_overwrite_their_flag_word():
    from anime_recommendations_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(34)
    n_users, n_anime = 301, 33
    u = np.repeat(np.arange(n_users), 9).astype(np.int32)
    a = np.concatenate([rng.choice(n_anime, 9, replace=False) for _ in range(n_users)]).astype(np.int32)
    r = (rng.integers(0, 11, len(u)) / 10).astype(np.float64)
    thr_o, fav_o = recs_oracle.favourites(u, a, r, n_users, 80)
    want = np.zeros((n_users, n_anime), bool)
    for uu in range(n_users):
        want[uu, sorted(fav_o[uu])] = True
    tu, ta, tr = (torch.as_tensor(x).cuda() for x in (u, a, r))
    for bad_row in (None, 5):
        aa = ta.clone()
        if bad_row is not None:
            aa[bad_row] = n_anime
        fav = poison.fill(torch.empty(n_users, 2, dtype=torch.int32, device="cuda"), 0x7F)
        thr = poison.fill(torch.empty(n_users, dtype=torch.float64, device="cuda"), 0x7F)
        err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x7F)
        ws = _dirty_ws(lib.anirec_fav_workspace_bytes(len(u), n_users))
        L.check(lib.anirec_user_favourites(L.ptr(tu), L.ptr(aa), L.ptr(tr), len(u), n_users, n_anime, 80.0, L.ptr(fav),
                                           L.ptr(thr), L.ptr(err), L.ptr(ws), ws.numel(), _stream()))
        if bad_row is None:
            assert err.item() == 0
            np.testing.assert_array_equal(fav.cpu().numpy().view(np.uint32), R.pack(want))
            assert np.array_equal(thr.cpu().numpy().view(np.uint64), thr_o.view(np.uint64))
        else:
            assert err.item() == 1
    cat = R.pack(rng.random((n_anime, 33)) < 0.2)
    tc = torch.from_numpy(cat.view(np.int32)).cuda()
    tf = torch.from_numpy(R.pack(want).view(np.int32)).cuda()
    for users in ([3, 0, 300, 17], [3, 301, 300, 17]):
        tus = torch.tensor(users, dtype=torch.int32).cuda()
        counts = poison.fill(torch.empty(len(users), 33, dtype=torch.int32, device="cuda"), 0x7F)
        err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x7F)
        L.check(lib.anirec_fave_profile(L.ptr(tf), n_users, n_anime, L.ptr(tus), len(users), L.ptr(tc), 33,
                                        L.ptr(counts), L.ptr(err), _stream()))
        if max(users) < n_users:
            assert err.item() == 0
            np.testing.assert_array_equal(counts.cpu().numpy(), R.fave_profile(R.pack(want), n_anime, cat, 33, users=users))
        else:
            assert err.item() == 1 and (counts[1] == 0).all()
