"""CPU tests of the item-kNN from co-occurrence: the restatement against literal Python loops on tiny inputs, the binding
and the entry points' refusals (no device needed), and the host logic of recs / components with ``ops`` replaced by the
restatement."""
import ctypes
import math
import os
import re
import struct

import numpy as np
import pytest

import cooc_restatement as R
from component_cli import load_component

from anime_recommendations_amd import _lib, build, components as C, data, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"anirec_cooc_chunk_words": 0, "anirec_cooc_workspace_bytes": 2, "anirec_cooc_scores": 16,
       "anirec_rows_topk_workspace_bytes": 3, "anirec_rows_topk": 13, "anirec_rows_rank": 11,
       "anirec_itemknn_lds_items": 0, "anirec_itemknn_workspace_bytes": 2, "anirec_itemknn_scores": 14}


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


# ---- the restatement against literal loops ----------------------------------------------------------------------------
def _liked(rng, n_items, n_users, density):
    return rng.random((n_items, n_users)) < density


def test_pack_and_unpack_bits_round_trip():
    rng = np.random.default_rng(0)
    for m in (1, 31, 32, 33, 70):
        M = _liked(rng, 5, m, 0.5)
        b = R.pack_bits(M)
        assert b.dtype == np.uint32 and b.shape == (5, (m + 31) // 32)
        for i in range(5):
            for u in range(m):
                assert bool((int(b[i, u >> 5]) >> (u & 31)) & 1) == bool(M[i, u])
        np.testing.assert_array_equal(R.unpack_bits(b, m), M)
        if m % 32:                                              # garbage past n_users is dropped
            b2 = b.copy()
            b2[:, -1] |= np.uint32((0xFFFFFFFF << (m % 32)) & 0xFFFFFFFF)
            np.testing.assert_array_equal(R.unpack_bits(b2, m), M)


@pytest.mark.parametrize("measure", [R.COSINE, R.JACCARD, R.CONFIDENCE])
@pytest.mark.parametrize("shrink,min_support", [(0.0, 0), (10.5, 1), (0.0, 3)])
def test_cooc_restatement_equals_literal_loops(measure, shrink, min_support):
    rng = np.random.default_rng(1)
    M = _liked(rng, 9, 37, 0.4)
    M[4] = False                                                # an item nobody liked
    M[7] = M[2]                                                 # twins
    queries = [2, 0, 9, 2, -1, 4, 8]
    sim, cnt, excl, pop, err = R.cooc_scores(R.pack_bits(M), 37, queries, measure, shrink, min_support)
    assert err == 1 and pop.tolist() == [int(r.sum()) for r in M]
    sets = [set(np.flatnonzero(r).tolist()) for r in M]
    E = R.unpack_bits(excl, 9)
    assert excl.shape == (len(queries), 1) and not (excl >> np.uint32(9)).any()
    for t, q in enumerate(queries):
        if not 0 <= q < 9:
            assert (_u32(sim[t]) == 0x7FC00000).all() and (cnt[t] == -1).all() and E[t].all()
            continue
        for j in range(9):
            c = len(sets[q] & sets[j])
            assert cnt[t, j] == c
            if measure == R.COSINE:
                den = math.sqrt(float(len(sets[q])) * float(len(sets[j]))) + shrink
            elif measure == R.JACCARD:
                den = float(len(sets[q] | sets[j])) + shrink
            else:
                den = float(len(sets[q])) + shrink
            ok = c >= max(1, min_support)
            want = _f32(c / den) if ok else 0.0
            assert sim[t, j] == want and not (want == 0.0 and np.signbit(sim[t, j]))
            assert E[t, j] == (not ok or j == q)
    np.testing.assert_array_equal(sim[0], sim[3])               # a repeated query
    if measure == R.COSINE and shrink == 0.0 and min_support <= 1:
        assert sim[0, 7] == 1.0 and sim[0, 2] == 1.0            # twins: exactly 1


def _key_py(x):
    """the documented order as a Python sort key: NaN last, larger first, +0 above -0"""
    if x != x:
        return (1, 0.0, 0)
    return (0, -x, 1 if (x == 0 and math.copysign(1, x) < 0) else 0)


def test_rows_topk_restatement_equals_a_python_sort():
    nan, inf = float("nan"), float("inf")
    S = np.array([[0.5, nan, -0.0, 0.0, 0.5, -inf, inf, 0.25, 0.0, -1.0, 7.0],
                  [nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, 7.0],
                  [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 7.0]], np.float32)
    n = 10                                                      # ld = 11: the last column must never be listed
    self_idx, keep = [6, -1, 0], np.array([1, 1, 1, 1, 0, 1, 1, 1, 1, 1], np.uint8)
    W = np.zeros((3, 10), bool)
    W[0, 7] = W[2, 3] = True
    for k in (1, 4, 10, 15):
        idx, sc = R.rows_topk(S, k, n, self_idx, keep, R.pack_bits(W))
        for t in range(3):
            cand = [j for j in range(n) if j != self_idx[t] and keep[j] and not W[t, j]]
            want = sorted(cand, key=lambda j: (_key_py(float(S[t, j])), j))[:k]
            assert idx[t, :len(want)].tolist() == want and (idx[t, len(want):] == -1).all()
            assert _u32(sc[t, :len(want)]).tolist() == _u32(S[t, want]).tolist()
            assert (_u32(sc[t, len(want):]) == 0x7FC00000).all()
    idx, _ = R.rows_topk(S, 10, n)
    assert idx[0].tolist() == [6, 0, 4, 7, 3, 8, 2, 9, 5, 1]


def test_rows_rank_restatement_is_the_position_in_the_full_list():
    rng = np.random.default_rng(2)
    S = rng.integers(0, 4, (5, 12)).astype(np.float32)
    S[1, 3] = np.nan
    S[2, 5], S[2, 6] = 0.0, -0.0
    W = rng.random((5, 12)) < 0.3
    tr, ta = np.repeat(np.arange(5), 12), np.tile(np.arange(12), 5)
    rank, err = R.rows_rank(S, 12, 12, R.pack_bits(W), 5, tr, ta)
    assert err == 0
    for t in range(len(tr)):
        w = W[tr[t]].copy()
        w[ta[t]] = False
        idx, _ = R.rows_topk(S[tr[t]:tr[t] + 1], 12, wbits=R.pack_bits(w[None]))
        assert idx[0, rank[t]] == ta[t]
    shared, err = R.rows_rank(S[0], 0, 12, R.pack_bits(W), 5, tr, ta)
    own, _ = R.rows_rank(np.tile(S[0], (5, 1)), 12, 12, R.pack_bits(W), 5, tr, ta)
    np.testing.assert_array_equal(shared, own)
    rank, err = R.rows_rank(S, 12, 12, None, 5, [0, 5, -1, 2], [12, 0, 0, 3])
    assert err == 1 and rank[:3].tolist() == [-1, -1, -1] and rank[3] >= 0


def test_itemknn_restatement_equals_literal_loops():
    rng = np.random.default_rng(3)
    n, K = 8, 3
    ni = rng.integers(-1, n, (n, K))
    ns = rng.random((n, K)).astype(np.float32)
    ns[1, 0], ni[1, 0] = 0.1, 2                                  # a term that is not a multiple of 2^-30
    off = [0, 4, 4, 7, 9]
    hi = [1, 1, 3, 0, 5, 6, 7, 2, 1]
    hw = rng.random(9).astype(np.float32) * 3
    for w in (None, hw):
        out, err = R.itemknn_scores(ni, ns, off, hi, w)
        assert err == 0 and out.shape == (4, n) and (out[1] == 0).all() and not np.signbit(out[1]).any()
        for l in range(4):
            S = [0] * n
            for e in range(off[l], off[l + 1]):
                for s in range(K):
                    j = int(ni[hi[e], s])
                    if j >= 0:
                        S[j] += round(float(1.0 if w is None else w[e]) * float(ns[hi[e], s]) * 2.0 ** 30)  # half-even
            assert out[l].tolist() == [_f32(v * 2.0 ** -30) for v in S]
    perm = [3, 2, 1, 0, 6, 5, 4, 8, 7]                          # entry order inside a list changes nothing
    again, _ = R.itemknn_scores(ni, ns, off, np.array(hi)[perm], hw[perm])
    assert again.tobytes() == R.itemknn_scores(ni, ns, off, hi, hw)[0].tobytes()
    ones, _ = R.itemknn_scores(ni, ns, off, hi, np.ones(9, np.float32))
    assert ones.tobytes() == R.itemknn_scores(ni, ns, off, hi, None)[0].tobytes()
    # every kind of bad value raises the flag and leaves the other lists as they were
    good = R.itemknn_scores(ni, ns, off, hi, hw)[0]
    for what in ("item", "neighbour", "offsets", "nan", "large"):
        ni2, ns2, off2, hi2, hw2 = ni.copy(), ns.copy(), list(off), list(hi), hw.copy()
        if what == "item":
            hi2[5] = n
        elif what == "neighbour":
            ni2[5, 1] = n
        elif what == "offsets":
            off2[2], off2[3] = 4, 3                             # list 2 is (4, 3): decreasing; list 3 becomes (3, 9)
        elif what == "nan":
            hw2[5] = np.nan
        else:
            hw2[5], ns2[5, :] = 2000.0, 0.75
        out, err = R.itemknn_scores(ni2, ns2, off2, hi2, hw2)
        assert err == 1, what
        assert out[0].tobytes() == good[0].tobytes() and out[1].tobytes() == good[1].tobytes(), what
        if what == "offsets":
            assert (_u32(out[2]) == 0x7FC00000).all()


# ---- the binding ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", code))
    for name, arity in NEW.items():
        assert name in declared and len(_lib.PROTOTYPES[name][1]) == arity, name
    assert "enum { ANIREC_COOC_COSINE = 0, ANIREC_COOC_JACCARD = 1, ANIREC_COOC_CONFIDENCE = 2 };" in code
    assert "#define ANIREC_ABI_VERSION 5" in src and _lib.ABI_VERSION == 5
    assert "anirec_seen_bits writes when it is called with the two index columns swapped" in src
    assert "anirec_cooc.hip" in build.SOURCES
    assert (_lib.COOC_COSINE, _lib.COOC_JACCARD, _lib.COOC_CONFIDENCE) == (R.COSINE, R.JACCARD, R.CONFIDENCE)
    assert _lib.COOC_MEASURES == R.MEASURES and tuple(_lib.COOC_MEASURES) == C.COOC_MEASURES
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.anirec_abi_version() == 5


def test_size_queries_and_refusals_need_no_device():
    build.build(verbose=False)
    lib = _lib.load()
    cw = lib.anirec_cooc_chunk_words()
    assert cw >= 4 and cw % 4 == 0
    assert lib.anirec_cooc_workspace_bytes(100, 7) >= 400 and lib.anirec_cooc_workspace_bytes(100, 0) >= 400
    assert lib.anirec_cooc_workspace_bytes(0, 7) == 0 and lib.anirec_cooc_workspace_bytes(100, -1) == 0
    fake = ctypes.c_void_p(4096)

    def cooc(n_items=10, n_users=40, nq=3, measure=0, shrink=0.0, min_support=1, p=fake, ws_bytes=1 << 20, **null):
        a = dict(bits=p, queries=p, sim=p, count=p, excl=p, pop=p, err=p, ws=p)
        a.update({k: None for k in null})
        return lib.anirec_cooc_scores(a["bits"], n_items, n_users, a["queries"], nq, measure, shrink, min_support, a["sim"],
                                      a["count"], a["excl"], a["pop"], a["err"], a["ws"], ws_bytes, None)
    for kw in (dict(n_items=0), dict(n_users=0), dict(nq=-1), dict(measure=3), dict(measure=-1), dict(shrink=-0.5),
               dict(shrink=float("nan")), dict(shrink=float("inf")), dict(min_support=-1)):
        assert cooc(**kw) == -1, kw
        assert cooc(**dict(kw, nq=0)) == -1 or "nq" in kw, kw   # a bad argument is refused whatever else the call holds
    assert cooc(nq=0, p=None) == 0                              # no query: nothing enqueued, nothing needed
    for name in ("bits", "queries", "sim", "err", "ws"):
        assert cooc(**{name: True}) == -1, name
    assert cooc(ws_bytes=lib.anirec_cooc_workspace_bytes(10, 3) - 1) == -3

    assert lib.anirec_rows_topk_workspace_bytes(0, 5, 10) == 0 and lib.anirec_rows_topk_workspace_bytes(100, -1, 10) == 0
    assert lib.anirec_rows_topk_workspace_bytes(100, 5, 0) == 0
    small, large = lib.anirec_rows_topk_workspace_bytes(1000, 5, 128), lib.anirec_rows_topk_workspace_bytes(1000, 5, 129)
    assert small > 0 and large > 0
    assert large < lib.anirec_topk_large_workspace_bytes(1000, 5, 129)     # no score rows in it

    def topk(ld=100, n=100, nq=3, k=10, p=fake, ws_bytes=1 << 30, **null):
        a = dict(scores=p, idx=p, score=p, ws=p)
        a.update({k_: None for k_ in null})
        return lib.anirec_rows_topk(a["scores"], ld, n, nq, None, None, None, k, a["idx"], a["score"], a["ws"], ws_bytes,
                                    None)
    for kw in (dict(n=0, ld=0), dict(nq=-1), dict(k=0), dict(ld=99)):
        assert topk(**kw) == -1, kw
    assert topk(nq=0, p=None) == 0
    for name in ("scores", "idx", "score", "ws"):
        assert topk(**{name: True}) == -1, name
    assert topk(ws_bytes=16) == -3 and topk(k=500, n=1000, ld=1000, ws_bytes=16) == -3

    def rank(ld=100, n=100, n_users=4, n_t=3, p=fake, **null):
        a = dict(scores=p, tr=p, ta=p, rank=p, err=p)
        a.update({k: None for k in null})
        return lib.anirec_rows_rank(a["scores"], ld, n, None, n_users, a["tr"], a["ta"], n_t, a["rank"], a["err"], None)
    for kw in (dict(n=0, ld=0), dict(n_users=-1), dict(n_t=-1), dict(ld=99), dict(ld=-1)):
        assert rank(**kw) == -1, kw
    assert rank(n_t=0, p=None) == 0
    for name in ("scores", "tr", "ta", "rank", "err"):
        assert rank(**{name: True}) == -1, name

    lds = lib.anirec_itemknn_lds_items()
    assert lds >= 1024
    assert lib.anirec_itemknn_workspace_bytes(0, 5) == 0 and lib.anirec_itemknn_workspace_bytes(10, -1) == 0
    assert 0 < lib.anirec_itemknn_workspace_bytes(lds, 5) < lds * 8
    assert lib.anirec_itemknn_workspace_bytes(lds + 1, 5) == (lds + 1) * 5 * 8

    def knn(n_items=10, K=4, n_lists=3, n_hist=9, p=fake, ws_bytes=1 << 20, **null):
        a = dict(ni=p, ns=p, off=p, hi=p, out=p, err=p, ws=p)
        a.update({k: None for k in null})
        return lib.anirec_itemknn_scores(a["ni"], a["ns"], n_items, K, a["off"], a["hi"], None, n_lists, n_hist, a["out"],
                                         a["err"], a["ws"], ws_bytes, None)
    for kw in (dict(n_items=0), dict(K=0), dict(n_lists=-1), dict(n_hist=-1)):
        assert knn(**kw) == -1, kw
    assert knn(n_lists=0, p=None) == 0
    for name in ("ni", "ns", "off", "hi", "out", "err", "ws"):
        assert knn(**{name: True}) == -1, name
    assert knn(n_items=lds + 1, ws_bytes=(lds + 1) * 3 * 8 - 1) == -3


def test_ops_checks_need_no_device():
    assert ops.check_cooc("Cosine", 0, 0) == (0, 0.0, 0) and ops.check_cooc(" jaccard ", 10.5, 3) == (1, 10.5, 3)
    assert ops.cooc_measure("CONFIDENCE") == 2
    with pytest.raises(ValueError, match="cosine, jaccard, confidence"):
        ops.cooc_measure("dice")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="shrink"):
            ops.check_cooc("cosine", bad, 1)
    with pytest.raises(ValueError, match="min_support"):
        ops.check_cooc("cosine", 0.0, -1)


# ---- host logic with ops replaced by the restatement -----------------------------------------------------------------
@pytest.fixture
def host_ops(monkeypatch):
    """``ops``' item-kNN wrappers (and seen_bits / score_rank / predict_rank) as the restatement on CPU tensors; the
    calls made are logged."""
    import torch
    calls = []

    def t(x):
        return None if x is None else torch.as_tensor(np.ascontiguousarray(x))

    def n(x):
        return None if x is None else (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))

    def seen_bits(u, a, n_users, n_anime, device=None):
        calls.append("seen_bits")
        return t(R.ops_seen_bits(n(u), n(a), n_users, n_anime))

    def cooc_scores(bits, n_users, queries, measure="cosine", shrink=0.0, min_support=1, count=False, excl=False,
                    pop=False, **kw):
        calls.append("cooc_scores")
        return tuple(t(x) for x in R.ops_cooc_scores(n(bits), n_users, n(queries), measure, shrink, min_support, count,
                                                     excl, pop))

    def rows_topk(scores, k, n_=None, self_idx=None, keep=None, wbits=None, **kw):
        calls.append("rows_topk")
        return tuple(t(x) for x in R.ops_rows_topk(n(scores), k, n_, n(self_idx), n(keep), n(wbits)))

    def rows_rank(scores, tr, ta, watched_bits=None):
        calls.append("rows_rank")
        return t(R.ops_rows_rank(n(scores), n(tr), n(ta), n(watched_bits)))

    def itemknn_scores(ni, ns, off, hi, hw=None, **kw):
        calls.append("itemknn_scores")
        return t(R.ops_itemknn_scores(n(ni), n(ns), n(off), n(hi), n(hw)))

    def score_rank(score, n_users, tr, ta, watched_bits=None):
        calls.append("score_rank")
        return t(R.rows_rank(n(score), 0, len(n(score)), n(watched_bits), n_users, n(tr), n(ta))[0])

    def predict_rank(U, A, head, users, tr, ta, watched_bits=None):
        calls.append("predict_rank")
        r = (np.asarray(n(tr)) * 7 + np.asarray(n(ta)) * 3) % 11
        return t(r.astype(np.int32)), t(np.zeros(len(r), np.float32))

    def listed_seen_bits(user_idx, anime_idx, users, n_users, n_anime, device=None):
        users = np.asarray(users)
        pos = {int(u): i for i, u in enumerate(users)}
        u, a = n(user_idx), n(anime_idx)
        take = np.isin(u, users)
        return t(R.ops_seen_bits([pos[int(x)] for x in u[take]], a[take], len(users), n_anime))

    for name, fn in dict(seen_bits=seen_bits, cooc_scores=cooc_scores, rows_topk=rows_topk, rows_rank=rows_rank,
                         itemknn_scores=itemknn_scores, score_rank=score_rank, predict_rank=predict_rank).items():
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(recs, "listed_seen_bits", listed_seen_bits)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self)
    return calls


def _frames():
    import pandas as pd
    ids = [10, 20, 30, 40, 50, 60]
    anime_df = pd.DataFrame({
        "anime_id": ids, "Name": ["a", "b", "c", "d", "e", "f"], "eng_version": ["a", "b", "c", "d", "e", "f"],
        "Genres": ["Action, Comedy", "Action", "Drama", "Comedy", "Action", "Drama"], "Episodes": ["1"] * 6,
        "japanese_name": ["x"] * 6, "Studios": ["s"] * 6, "Premiered": ["p"] * 6, "Score": ["7"] * 6,
        "Type": ["TV", "TV", "Movie", "TV", "OVA", "TV"], "Source": ["Manga"] * 6, "Rating": ["PG"] * 6})
    syn_df = pd.DataFrame({"MAL_ID": ids, "sypnopsis": ["syn %d" % i for i in ids]})
    rng = np.random.default_rng(5)
    L = rng.random((30, 6)) < 0.5
    L[:, 0] = True
    u, a = np.nonzero(L)
    order = rng.permutation(len(u))
    df = pd.DataFrame({"user_id": u[order] + 1000, "anime_id": np.asarray(ids)[a[order]],
                       "rating": rng.integers(1, 11, len(u)) / 10.0})
    return df, anime_df, syn_df


def test_also_liked_frame_host_logic(host_ops):
    df, anime_df, syn_df = _frames()
    frame, fn = C.also_liked_frame(df, anime_df, syn_df, "a", 4)
    assert fn == "a_also_liked.csv" and host_ops == ["seen_bits", "cooc_scores", "rows_topk"]
    assert frame.columns.tolist() == ["Name", "Similarity", "Genres", "Sypnopsis", "Episodes", "Japanese name", "Studios",
                                      "Premiered", "Score", "Type", "Source", "Rating", "Liked_by_both", "Liked_by"]
    # the definition, on the frame itself: users who rated both / sqrt(raters of a x raters of the other)
    by = {aid: set(g.user_id) for aid, g in df.groupby("anime_id")}
    name_of = dict(zip(anime_df.anime_id, anime_df.Name))
    order = C.index_tables({}, df)[1].tolist()                  # ties: the anime index, order of first appearance
    want = sorted(((len(by[10] & by[x]) / math.sqrt(len(by[10]) * len(by[x])), name_of[x]) for x in order if x != 10),
                  key=lambda p: -p[0])[:4]
    assert frame["Name"].tolist() == [w[1] for w in want]
    assert frame["Similarity"].tolist() == [_f32(w[0]) for w in want]
    ids = {v: k for k, v in name_of.items()}
    assert frame["Liked_by_both"].tolist() == [len(by[10] & by[ids[x]]) for x in frame["Name"]]
    assert frame["Liked_by"].tolist() == [len(by[ids[x]]) for x in frame["Name"]]
    assert not (frame["Name"] == "a").any()
    # filters, the threshold and the support narrow the list; a huge count is every other anime
    tv = C.also_liked_frame(df, anime_df, syn_df, "a", 100, types=["TV"])[0]
    assert set(tv["Name"]) == {"b", "d", "f"}
    act = C.also_liked_frame(df, anime_df, syn_df, "a", 100, genres=["Action"])[0]
    assert set(act["Name"]) == {"b", "e"}
    hi = C.also_liked_frame(df, anime_df, syn_df, "a", 100, liked_min_rating=0.6, measure="jaccard")[0]
    liked = df[df.rating.astype(np.float32) >= np.float32(0.6)]
    by6 = {aid: set(g.user_id) for aid, g in liked.groupby("anime_id")}
    for _, r in hi.iterrows():
        x = ids[r["Name"]]
        assert r["Liked_by_both"] == len(by6[10] & by6[x]) and r["Similarity"] == _f32(len(by6[10] & by6[x]) / len(by6[10] | by6[x]))
    assert len(C.also_liked_frame(df, anime_df, syn_df, "a", 100, min_support=1000)[0]) == 0
    conf = C.also_liked_frame(df, anime_df, syn_df, "b", 2, measure="confidence", shrink=10.5)[0]
    assert conf["Similarity"].tolist() == sorted(conf["Similarity"], reverse=True)
    assert conf["Similarity"][0] == _f32(conf["Liked_by_both"][0] / (len(by[20]) + 10.5))
    with pytest.raises(ValueError, match="cosine, jaccard, confidence"):
        C.also_liked_frame(df, anime_df, syn_df, "a", 4, measure="dice")
    with pytest.raises(ValueError, match="not found"):
        C.also_liked_frame(df, anime_df, syn_df, "zzz", 4)
    with pytest.raises(ValueError, match="a_query_number"):
        C.also_liked_frame(df, anime_df, syn_df, "a", 0)
    with pytest.raises(ValueError, match="no rating"):
        C.also_liked_frame(df[df.anime_id != 60], anime_df, syn_df, "f", 4)


def _table(n_users=40, n_anime=25, n=900, seed=6):
    rng = np.random.default_rng(seed)
    pairs = rng.permutation(n_users * n_anime)[:n]
    return data.RatingTable(pairs // n_anime, pairs % n_anime, rng.integers(1, 11, n) / 10.0, np.arange(n_users) + 100,
                            np.arange(n_anime) + 500)


def _model(table):
    head = dict(w=1.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0)
    return dict(U=np.zeros((table.n_users, 32), np.float32), A=np.zeros((table.n_anime, 32), np.float32), head=head,
                user_ids=table.user_ids, anime_ids=table.anime_ids)


def test_evaluate_frame_without_itemknn_is_as_it_was(host_ops):
    table = _table()
    model = _model(table)
    keys = ["n", "n_users", "test_size", "min_rating", "mrr", "mean_rank", "median_rank", "hit_rate@1", "ndcg@1",
            "hit_rate@5", "ndcg@5"]
    plain, plain_summary = C.evaluate_frame(model, table, 200, [5, 1], 0.5)
    assert plain.columns.tolist() == ["k", "hit_rate", "ndcg"] and list(plain_summary) == keys and plain_summary["n"] > 50
    none, none_summary = C.evaluate_frame(model, table, 200, [5, 1], 0.5, baseline=None)
    assert none.to_csv(index=False) == plain.to_csv(index=False) and none_summary == plain_summary
    assert "cooc_scores" not in host_ops and "itemknn_scores" not in host_ops and "score_rank" not in host_ops
    users, row, anime, train = recs.held_out_targets(table, 200, 0.5)
    want = recs.ranking_metrics((row * 7 + anime * 3) % 11, [1, 5])           # the stub's ranks
    assert plain["hit_rate"].tolist() == [want["hit_rate"][1], want["hit_rate"][5]] and plain_summary["mrr"] == want["mrr"]
    pop, pop_summary = C.evaluate_frame(model, table, 200, [5, 1], 0.5, baseline="popularity")
    assert pop.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity"]
    assert list(pop_summary) == keys + ["popularity_mrr", "popularity_mean_rank", "popularity_hit_rate@1",
                                        "popularity_ndcg@1", "popularity_hit_rate@5", "popularity_ndcg@5"]
    assert pop[["k", "hit_rate", "ndcg"]].to_csv(index=False) == plain.to_csv(index=False)
    as_list = C.evaluate_frame(model, table, 200, [5, 1], 0.5, baseline=["popularity"])
    assert as_list[0].to_csv(index=False) == pop.to_csv(index=False) and as_list[1] == pop_summary
    assert "cooc_scores" not in host_ops and "itemknn_scores" not in host_ops
    # the popularity ranks, from the definition
    counts = np.bincount(table.anime[train], minlength=table.n_anime)
    seen = np.zeros((table.n_users, table.n_anime), bool)
    seen[table.user[train], table.anime[train]] = True
    r = []
    for u, a in zip(users[row], anime):
        before = (counts > counts[a]) | ((counts == counts[a]) & (np.arange(table.n_anime) < a))
        r.append(int((before & ~seen[u] & (np.arange(table.n_anime) != a)).sum()))
    b = recs.ranking_metrics(r, [1, 5])
    assert pop_summary["popularity_mrr"] == b["mrr"] and pop["ndcg_popularity"].tolist() == [b["ndcg"][1], b["ndcg"][5]]


def test_evaluate_frame_itemknn_host_logic(host_ops):
    table = _table()
    model = _model(table)
    par = dict(neighbours=4, measure="jaccard", shrink=0.5, min_support=2, min_rating=0.4)
    frame, summary = C.evaluate_frame(model, table, 200, [1, 5], 0.5, baseline="itemknn", itemknn=par)
    assert frame.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_itemknn", "ndcg_itemknn"]
    assert list(summary)[-6:] == ["itemknn_mrr", "itemknn_mean_rank", "itemknn_hit_rate@1", "itemknn_ndcg@1",
                                  "itemknn_hit_rate@5", "itemknn_ndcg@5"]
    assert "score_rank" not in host_ops and {"cooc_scores", "rows_topk", "itemknn_scores", "rows_rank"} <= set(host_ops)
    # the same figures from the restatement alone, fitted on the TRAINING slice
    users, row, anime, train = recs.held_out_targets(table, 200, 0.5)
    tu, ta, tr = table.user[train], table.anime[train], table.rating[train].astype(np.float32)
    liked = tr >= np.float32(0.4)
    L = np.zeros((table.n_anime, table.n_users), bool)
    L[ta[liked], tu[liked]] = True
    sim, _, excl, _, _ = R.cooc_scores(R.pack_bits(L), table.n_users, np.arange(table.n_anime), R.JACCARD, 0.5, 2)
    ni, ns = R.rows_topk(sim, 4, wbits=excl)
    off = np.concatenate([[0], np.cumsum([int(((tu == u) & liked).sum()) for u in users])])
    hist = np.concatenate([ta[(tu == u) & liked] for u in users])
    scores, err = R.itemknn_scores(ni, ns, off, hist)
    seen = np.zeros((len(users), table.n_anime), bool)
    for i, u in enumerate(users):
        seen[i, ta[tu == u]] = True
    rank, err2 = R.rows_rank(scores, table.n_anime, table.n_anime, R.pack_bits(seen), len(users), row, anime)
    assert err == 0 and err2 == 0
    b = recs.ranking_metrics(rank, [1, 5])
    assert summary["itemknn_mrr"] == b["mrr"] and summary["itemknn_mean_rank"] == b["mean_rank"]
    assert frame["hit_rate_itemknn"].tolist() == [b["hit_rate"][1], b["hit_rate"][5]]
    assert frame["ndcg_itemknn"].tolist() == [b["ndcg"][1], b["ndcg"][5]]
    both, both_summary = C.evaluate_frame(model, table, 200, [1, 5], 0.5, baseline=("itemknn", "popularity"), itemknn=par)
    assert both.columns.tolist() == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity", "hit_rate_itemknn",
                                     "ndcg_itemknn"]
    assert both["ndcg_itemknn"].tolist() == frame["ndcg_itemknn"].tolist()
    assert both_summary["itemknn_mrr"] == summary["itemknn_mrr"] and "popularity_mrr" in both_summary
    for wrong in ("ItemKNN", "none", ["popularity", "knn"], ""):
        with pytest.raises(ValueError, match="baseline"):
            C.evaluate_frame(model, table, 200, [1], 0.5, baseline=wrong)
    with pytest.raises(ValueError, match="itemknn parameter"):
        C.evaluate_frame(model, table, 200, [1], 0.5, baseline="itemknn", itemknn={"k": 3})
    # batches of lists change nothing
    knn = dict(nbr_idx=__import__("torch").as_tensor(ni), nbr_sim=__import__("torch").as_tensor(ns))
    r1 = recs.itemknn_rank(knn, off, hist, None, R.pack_bits(seen).view(np.int32), row, anime, batch=3)
    np.testing.assert_array_equal(r1.numpy(), rank)
    i1, s1 = recs.itemknn_topk(knn, off, hist, None, 6, R.pack_bits(seen).view(np.int32), batch=5)
    i2, s2 = R.rows_topk(scores, 6, wbits=R.pack_bits(seen))
    np.testing.assert_array_equal(i1.numpy(), i2)
    assert s1.numpy().tobytes() == s2.tobytes()


# ---- the components' flag surfaces ---------------------------------------------------------------------------------
def test_also_liked_parser_and_mlproject_agree():
    mod = load_component("also_liked")
    sim = load_component("similar_anime")
    model_flags = {"model_type", "model", "ID_emb_name", "anime_emb_name"}
    assert mod.STR_FLAGS == [f for f in sim.STR_FLAGS if f not in model_flags] and mod.BOOL_FLAGS == sim.BOOL_FLAGS
    assert mod.OPTIONAL_FLAGS == {"liked_min_rating": 0.0, "cooc_measure": "cosine", "cooc_shrink": 0.0,
                                  "cooc_min_support": 1}
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert {f: getattr(ns, f) for f in mod.OPTIONAL_FLAGS} == mod.OPTIONAL_FLAGS
    assert sorted(vars(ns)) == sorted(mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS))
    ns = parser.parse_args(argv + ["--liked_min_rating", "0.7", "--cooc_measure", " Jaccard", "--cooc_shrink", "10.5",
                                   "--cooc_min_support", "3"])
    assert (ns.liked_min_rating, ns.cooc_measure, ns.cooc_shrink, ns.cooc_min_support) == (0.7, "jaccard", 10.5, 3)
    for bad in (["--liked_min_rating", "1.5"], ["--liked_min_rating", "x"], ["--cooc_measure", "dice"],
                ["--cooc_shrink", "-1"], ["--cooc_shrink", "inf"], ["--cooc_min_support", "-1"],
                ["--cooc_min_support", "1.5"], ["--save_sim_anime", "maybe"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "also_liked", "MLproject")))
    assert ml["name"] == "also_liked" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS)
    assert all(v["description"] for v in params.values())
    for f, v in params.items():
        if f in mod.OPTIONAL_FLAGS:
            assert getattr(mod, f)(v["default"]) == mod.OPTIONAL_FLAGS[f]
        else:
            assert v["type"] == "str" and "default" not in v
    assert main["command"] == "python also_liked.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert yaml.safe_load(open(os.path.join(ROOT, "also_liked", "conda.yml")))["name"] == "also_liked"


def test_evaluate_baseline_flag_takes_names_and_lists():
    mod = load_component("evaluate")
    assert mod.baseline_arg("none") is None and mod.baseline_arg(" None ") is None and mod.baseline_arg("") is None
    assert mod.baseline_arg("popularity") == ["popularity"] and mod.baseline_arg("ItemKNN") == ["itemknn"]
    assert mod.baseline_arg("popularity, itemknn") == ["popularity", "itemknn"]
    assert C.baseline_names(None) == () and C.baseline_names("itemknn") == ("itemknn",)
    assert C.baseline_names(["itemknn", "popularity", "itemknn"]) == ("popularity", "itemknn")
    assert C.BASELINES == ("popularity", "itemknn")
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    ns = mod.make_cli_parser().parse_args(argv)
    got = {f[len("itemknn_"):]: getattr(ns, f) for f in mod.ITEMKNN_FLAGS}
    assert got == C.ITEMKNN_DEFAULTS and ns.baseline == "none"
    ns = mod.make_cli_parser().parse_args(argv + ["--baseline", "popularity,itemknn", "--itemknn_neighbours", "20",
                                                   "--itemknn_measure", "jaccard", "--itemknn_shrink", "10.5",
                                                   "--itemknn_min_support", "3", "--itemknn_min_rating", "0.7"])
    assert (ns.itemknn_neighbours, ns.itemknn_measure, ns.itemknn_shrink, ns.itemknn_min_support,
            ns.itemknn_min_rating) == (20, "jaccard", 10.5, 3, 0.7)
    assert not any(hasattr(mod.make_parser().parse_args(argv), f) for f in mod.ITEMKNN_FLAGS)
