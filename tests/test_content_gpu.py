"""GPU tests of the content-based system (anirec_content_scores; ops / recs wrappers; the content_recs component,
evaluate --baseline content and content as a hybrid_recs member).

Yardstick: the NumPy restatement (tests/content_restatement.py).  Every comparison is exact, on bits, NaNs included; there
is no tolerance anywhere: the profile is an int64 sum of fixed-point terms, its image one correctly rounded divide, a
score a fixed fp32 fma chain in storage order.

Shapes: item counts around the 256 items a workgroup's threads take per pass and past several passes; token counts of
one, below a wave, past a pass of the image loop, and on both sides of the two switches between the kernel's three
forms (anirec_content_lds_tokens and twice that) with a sparse vocabulary; one list and 130; histories that are empty, of one and of nine
entries, of 2 000 with repeats, of items without tokens, with negative and with all-zero weights."""
import ctypes
import json

import numpy as np
import pandas as pd
import pytest

import content_restatement as R
import cooc_restatement as CR
import poison
import recs_fixture as RF
from als_restatement import fma_exact
from test_content_cpu import _meta, check_planted, planted
from test_cooc_gpu import fixture_store  # noqa: F401  (the recs fixture as an artifact store)
from test_fuse_gpu import _mr_flags
from test_rank_gpu import _run as _run_out
from test_recs_fixtures_gpu import _run

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
N_ITEMS = (1, 255, 256, 257, 1000)
N_TOKENS = (1, 63, 300, "lds", "lds+1", "2lds", "2lds+1")    # the last four: both sides of either switch of form
N_LISTS = 130


def _cuda(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _u32(x):
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    return np.ascontiguousarray(a).view(np.uint32)


def _lds():
    from anime_recommendations_amd import _lib
    return int(_lib.load().anirec_content_lds_tokens())


def _n_tokens(case):
    return {"lds": _lds(), "lds+1": _lds() + 1, "2lds": 2 * _lds(), "2lds+1": 2 * _lds() + 1}.get(case, case)


def _case(n_items, n_tokens, seed, n_lists=N_LISTS, long_history=2000):
    """(item CSR, history CSR with weights): rows of 0 .. 8 slots (an empty row and a repeated token among them) over a
    vocabulary of which few ids occur (the first and the last do); the lists the module docstring names, then random"""
    rng = np.random.default_rng(seed)
    used = np.unique(np.concatenate([[0, n_tokens - 1], rng.integers(0, n_tokens, 40)]))
    lens = rng.integers(0, 9, n_items)
    if n_items >= 3:
        lens[1], lens[2] = 0, 4
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.choice(used, int(off[-1])).astype(np.int32)
    w = (rng.random(int(off[-1])) * 1.5 - 0.25).astype(np.float32)
    if n_items >= 3:
        idx[off[2] + 1] = idx[off[2]]                                   # a repeated token
    empty = np.flatnonzero(lens == 0)
    hists = [[], [n_items - 1], rng.integers(0, n_items, 9), rng.integers(0, min(n_items, 50), long_history),
             np.repeat(empty, 3) if len(empty) else [], rng.integers(0, n_items, 12), rng.integers(0, n_items, 7)]
    hists += [rng.integers(0, n_items, rng.integers(0, 21)) for _ in range(n_lists - len(hists))]
    hists = [np.asarray(h, np.int32) for h in hists[:n_lists]]
    ws = [(rng.integers(1, 11, len(h)) / 10.0) for h in hists]
    if n_lists > 6:
        ws[5] = -ws[5] * (rng.random(len(ws[5])) < 0.6)                 # negative (and some zero) weights
        ws[6] = ws[6] * 0.0                                             # all-zero weights: a zero row
    hoff = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int32)
    return (off, idx, w), (hoff, np.concatenate(hists).astype(np.int32), np.concatenate(ws).astype(np.float32))


def _gpu(csr, n_tokens, hoff, hist, hw, **kw):
    from anime_recommendations_amd import ops
    return ops.content_scores(_cuda(csr[0]), _cuda(csr[1]), _cuda(csr[2]), n_tokens, hoff, hist, hw, **kw)


# ---- bit-equality with the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", N_TOKENS)
@pytest.mark.parametrize("n_items", N_ITEMS)
def test_scores_equal_the_restatement(n_items, tokens):
    n_tokens = _n_tokens(tokens)
    csr, (hoff, hist, hw) = _case(n_items, n_tokens, 100 + n_items)
    want, err = R.content_scores(*csr, n_tokens, hoff, hist, hw)
    assert err == 0 and want.shape == (N_LISTS, n_items)
    got = _gpu(csr, n_tokens, hoff, hist, hw)
    assert np.array_equal(_u32(got), _u32(want))
    assert not (_u32(got)[[0, 6]]).any()                                # no history, all-zero weights: +0 everywhere
    plain, err = R.content_scores(*csr, n_tokens, hoff, hist, None)
    assert err == 0 and np.array_equal(_u32(_gpu(csr, n_tokens, hoff, hist, None)), _u32(plain))
    # n_lists = 1: a list alone is its row inside the batch of 130
    for l in (0, 1, 2, 3, 5, 6, 77):
        alone = _gpu(csr, n_tokens, [0, hoff[l + 1] - hoff[l]], hist[hoff[l]:hoff[l + 1]], hw[hoff[l]:hoff[l + 1]])
        assert alone.shape == (1, n_items) and np.array_equal(_u32(alone)[0], _u32(want)[l]), l
    perm = np.random.default_rng(1).permutation(int(hoff[4] - hoff[3])) + hoff[3]       # entry order changes nothing
    again = _gpu(csr, n_tokens, [0, len(perm)], hist[perm], hw[perm])
    assert np.array_equal(_u32(again)[0], _u32(want)[3])
    assert _gpu(csr, n_tokens, [0], hist, hw).shape == (0, n_items)                     # no list


@pytest.mark.parametrize("tokens", [300, "lds+1", "2lds+1"])
def test_result_ignores_what_workspace_and_outputs_held(tokens):
    n_tokens = _n_tokens(tokens)
    csr, (hoff, hist, hw) = _case(257, n_tokens, 7, n_lists=9, long_history=300)
    want, _ = R.content_scores(*csr, n_tokens, hoff, hist, hw)
    dev = [_cuda(x) for x in csr]
    from anime_recommendations_amd import ops
    for byte in poison.ORDER:
        log = []
        with poison.poisoned(byte, log):
            got = ops.content_scores(*dev, n_tokens, hoff, hist, hw)
        assert len(log) >= 2 and max(log) >= 9 * 257 * 4                # the outputs and the workspace were dirty
        if tokens != 300:
            assert max(log) >= 9 * n_tokens * 8                         # the global form's rows among them
        assert np.array_equal(_u32(got), _u32(want)), hex(byte)


@pytest.mark.parametrize("tokens", [300, "lds+1", "2lds+1"])
def test_bad_values_raise_the_flag_and_spare_the_other_rows(tokens):
    from anime_recommendations_amd import ops
    n_tokens = _n_tokens(tokens)
    csr, (hoff, hist, hw) = _case(257, n_tokens, 8, n_lists=9, long_history=300)
    clean = _gpu(csr, n_tokens, hoff, hist, hw)
    assert np.array_equal(_u32(clean), _u32(R.content_scores(*csr, n_tokens, hoff, hist, hw)[0]))
    e = int(hoff[2]) + 4                                                # an entry of list 2 (nine entries)
    for what in ("item", "negative item", "offsets", "nan", "inf", "large entry", "large term", "token", "token nan"):
        (off, idx, w), hoff2, hist2, hw2 = [x.copy() for x in csr], hoff.copy(), hist.copy(), hw.copy()
        if what == "item":
            hist2[e] = 257
        elif what == "negative item":
            hist2[e] = -1
        elif what == "offsets":
            hoff2[3] = hoff2[2] - 1                                     # list 2 is decreasing, list 3 starts earlier
        elif what == "nan":
            hw2[e] = np.nan
        elif what == "inf":
            hw2[e] = -np.inf
        elif what == "large entry":
            hw2[e] = 1025.0
        elif what == "large term":
            top = int(np.argmax(w))
            assert w[top] > 1.0
            hw2[e], hist2[e] = 1024.0, int(np.searchsorted(off, top, "right") - 1)     # the entry passes, 1024 x w[top] not
        elif what == "token":
            idx[off[2] + 2] = n_tokens
        else:
            w[off[2] + 2] = np.nan
        want, err = R.content_scores(off, idx, w, n_tokens, hoff2, hist2, hw2)
        assert err == 1, what
        got, flag = _gpu((off, idx, w), n_tokens, hoff2, hist2, hw2, check=False)
        assert int(flag.item()) == 1, what
        assert np.array_equal(_u32(got), _u32(want)), what
        with pytest.raises(ValueError, match="out of range"):
            _gpu((off, idx, w), n_tokens, hoff2, hist2, hw2)
        others = [l for l in range(9) if l != 2 and not (what == "offsets" and l == 3)]
        if what.startswith("token"):        # the clean call is the one with that slot's weight 0: the slot adds nothing
            idx[off[2] + 2], w[off[2] + 2] = 0, 0.0
            zero, flag = _gpu((off, idx, w), n_tokens, hoff, hist, hw, check=False)
            assert int(flag.item()) == 0 and np.array_equal(_u32(got), _u32(zero)), what
        else:
            assert len(others) >= 6 and np.array_equal(_u32(got)[others], _u32(clean)[others]), what
        if what == "offsets":
            assert (_u32(got)[2] == NAN_BITS).all()
    with pytest.raises(ValueError, match="rise from 0"):                # the item CSR itself, checked on the way in
        _gpu((csr[0][::-1].copy(), csr[1], csr[2]), n_tokens, hoff, hist, hw)


# ---- the cosine, the recs layer ---------------------------------------------------------------------------------------
def test_one_entry_history_is_the_cosine_of_two_tfidf_rows():
    from anime_recommendations_amd import ops, recs
    meta = pd.concat([_meta()] * 3, ignore_index=True)
    meta.loc[7, "Genres"] = "Drama, Action"
    fit = recs.content_fit(meta, recs.CONTENT_COLUMNS + ("Sypnopsis",))
    off, ti, tw = (fit[k].cpu().numpy() for k in ("tok_offsets", "tok_idx", "tok_w"))
    n, T = fit["n_items"], fit["n_tokens"]
    got = ops.content_scores(fit["tok_offsets"], fit["tok_idx"], fit["tok_w"], T, np.arange(n + 1), np.arange(n))
    got = got.cpu().numpy()
    for q in range(n):
        # restated from the rule alone: Wq = 2^30, P = rint(x 2^30), the chain over the other row
        p = np.zeros(T, np.float32)
        p[ti[off[q]:off[q + 1]]] = (np.rint(tw[off[q]:off[q + 1]].astype(np.float64) * 2.0 ** 30) / 2.0 ** 30).astype(np.float32)
        for j in range(n):
            acc = np.zeros(1, np.float32)
            for t in range(off[j], off[j + 1]):
                acc = fma_exact(p[ti[t]:ti[t] + 1], tw[t:t + 1], acc)
            assert got[q, j] == acc[0], (q, j)
            dense = np.zeros(T)
            dense[ti[off[j]:off[j + 1]]] = tw[off[j]:off[j + 1]]
            assert abs(float(got[q, j]) - float(dense @ p.astype(np.float64))) < 1e-6
        if off[q + 1] > off[q]:
            assert abs(got[q, q] - 1.0) < 1e-6                          # unit rows
    # content_similar never lists the query, twins first
    idx, sim = recs.content_similar(fit, np.arange(n), 5)
    idx, sim = idx.cpu().numpy(), sim.cpu().numpy()
    assert not (idx == np.arange(n)[:, None]).any() and (idx >= 0).all()
    assert idx[0, :2].tolist() == [6, 12] and (np.abs(sim[0, :2] - 1.0) < 1e-6).all()
    keep = np.ones(n, np.uint8)
    keep[6] = 0
    assert recs.content_similar(fit, [0], 5, keep=keep)[0].cpu().numpy()[0, 0] == 12


def test_content_topk_and_rank_agree_with_the_row_ops():
    import torch
    from anime_recommendations_amd import ops, recs
    n_items, n_tokens = 300, 63
    csr, (hoff, hist, hw) = _case(n_items, n_tokens, 31, n_lists=40, long_history=100)
    fit = dict(tok_offsets=_cuda(csr[0]), tok_idx=_cuda(csr[1]), tok_w=_cuda(csr[2]), n_items=n_items, n_tokens=n_tokens)
    rng = np.random.default_rng(2)
    seen = _cuda(CR.pack_bits(rng.random((40, n_items)) < 0.2).view(np.int32))
    rows = ops.content_scores(fit["tok_offsets"], fit["tok_idx"], fit["tok_w"], n_tokens, hoff, hist, hw)
    assert np.array_equal(_u32(recs.content_rows_source(fit, hoff, hist, hw)(3, 17)), _u32(rows[3:17]))
    for batch in (7, recs.CONTENT_BATCH):
        i1, s1 = recs.content_topk(fit, hoff, hist, hw, 12, seen, batch=batch)
        i2, s2 = ops.rows_topk(rows, 12, wbits=seen)
        assert torch.equal(i1, i2) and np.array_equal(_u32(s1), _u32(s2))
        tr, ta = rng.integers(0, 40, 200), rng.integers(0, n_items, 200)
        r1 = recs.content_rank(fit, hoff, hist, hw, seen, tr, ta, batch=batch)
        assert torch.equal(r1, ops.rows_rank(rows, tr, ta, seen))
    want, _ = R.content_scores(*csr, n_tokens, hoff, hist, hw)
    wi, ws = CR.rows_topk(want, 12, wbits=seen.cpu().numpy().view(np.uint32))
    assert np.array_equal(i1.cpu().numpy(), wi) and np.array_equal(_u32(s1), _u32(ws))
    # the global form in spans: the batch shrinks so that the workspace stays under CONTENT_WS_BYTES
    big = dict(fit, n_tokens=1 << 22)
    assert recs.content_batch(big) == 32
    i3, s3 = recs.content_topk(big, hoff, hist, hw, 12, seen)
    assert torch.equal(i3, i1) and np.array_equal(_u32(s3), _u32(s1))


# ---- graph capture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [300, "lds+1", "2lds+1"])
def test_scores_and_select_replay_from_a_graph(tokens):
    """scores + select captured into one graph on one stream run nothing; the replay writes the restatement's bits"""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    n_tokens, n_items, n_l, k = _n_tokens(tokens), 257, 9, 10
    csr, (hoff, hist, hw) = _case(n_items, n_tokens, 9, n_lists=n_l, long_history=300)
    to, ti, tw, off, hi, w = (_cuda(x) for x in (*csr, hoff, hist, hw))
    shapes = ((n_l * n_items, torch.float32), (1, torch.int32), (n_l * k, torch.int32), (n_l * k, torch.float32))
    out, err, idx, val = [poison.fill(torch.empty(m, dtype=dt, device="cuda"), 0x3F) for m, dt in shapes]
    ws_a = poison.fill(torch.empty(int(lib.anirec_content_workspace_bytes(n_tokens, n_l)), dtype=torch.uint8, device="cuda"), 0x3F)
    ws_b = poison.fill(torch.empty(int(lib.anirec_rows_topk_workspace_bytes(n_items, n_l, k)), dtype=torch.uint8,
                                   device="cuda"), 0x3F)
    from anime_recommendations_amd import ops
    ops.content_scores(to, ti, tw, n_tokens, hoff, hist, hw)            # the kernel is loaded before the capture begins
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st_a = lib.anirec_content_scores(_lib.ptr(to), _lib.ptr(ti), _lib.ptr(tw), n_items, n_tokens, _lib.ptr(off),
                                         _lib.ptr(hi), _lib.ptr(w), n_l, len(hist), _lib.ptr(out), _lib.ptr(err),
                                         _lib.ptr(ws_a), ws_a.numel(), s)
        st_b = lib.anirec_rows_topk(_lib.ptr(out), n_items, n_items, n_l, None, None, None, k, _lib.ptr(idx),
                                    _lib.ptr(val), _lib.ptr(ws_b), ws_b.numel(), s)
    assert st_a == 0 and st_b == 0
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0x3F).all()) for t in (out, err, idx, val))         # captured, not run
    want, _ = R.content_scores(*csr, n_tokens, hoff, hist, hw)
    wi, wv = CR.rows_topk(want, k)
    graph.replay()
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and np.array_equal(_u32(out.view(n_l, n_items)), _u32(want))
    assert np.array_equal(idx.view(n_l, k).cpu().numpy(), wi) and np.array_equal(_u32(val.view(n_l, k)), _u32(wv))


# ---- the planted case -------------------------------------------------------------------------------------------------
def test_planted_families_on_the_gpu():
    from anime_recommendations_amd import recs
    (off, idx, w, n_tokens), (hoff, hist, hw), held, seen, nA = planted()
    got = _gpu((off, idx, w), n_tokens, hoff, hist, hw).cpu().numpy()
    want, _ = R.content_scores(off, idx, w, n_tokens, hoff, hist, hw)
    assert np.array_equal(_u32(got), _u32(want))
    check_planted(got, held, seen, nA)
    fit = dict(tok_offsets=_cuda(off), tok_idx=_cuda(idx), tok_w=_cuda(w), n_items=30, n_tokens=n_tokens)
    bits = _cuda(CR.pack_bits(seen).view(np.int32))
    rank = recs.content_rank(fit, hoff, hist, hw, bits, np.arange(16), held, batch=5).cpu().numpy()
    assert np.array_equal(rank, CR.rows_rank(want, 30, 30, CR.pack_bits(seen), 16, np.arange(16), held)[0])
    assert all(rank[u] < (nA if u % 2 == 0 else 30 - nA) - 6 for u in range(16))


# ---- the components, end to end on the recs fixture -------------------------------------------------------------------
def _fixture_frames(rec):
    from anime_recommendations_amd import components as C
    return C.load_anime_df(RF.csv(rec, "anime_csv")), C.load_synopses(RF.csv(rec, "synopses_csv"))


def _cr_flags(flags, **kw):
    return dict(dict(project_name="anime_recommendations", main_df="user_stats.parquet:latest", main_df_type="parquet",
                     anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopses_df="synopses.csv:latest",
                     sypnopsis_df_type="raw_data", anime_query="none", a_query_number=20, random_anime=False,
                     anime_rec_genres=flags["SA_GENRES"], an_spec_genres=False, types=flags["SA_TYPES"], spec_types=False,
                     a_rec_type="csv", save_sim_anime=True), **kw)


def test_content_recs_component_for_an_anime_nobody_rated(fixture_store):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, recs
    work, env, rec, df = (fixture_store[k] for k in ("work", "env", "rec", "df"))
    anime_df, syn_df = _fixture_frames(rec)
    ids = C.content_universe(anime_df)
    unrated = anime_df[~anime_df.anime_id.isin(set(df.anime_id))]
    assert len(unrated) >= 1 and len(ids) > df.anime_id.nunique()
    query = str(unrated["Name"].iloc[0])
    _run("content_recs", _cr_flags(rec["flags"], anime_query=query, spec_types=True), str(work), env)
    fn = C.clean(query) + "_content.csv"
    got = (work / fn).read_text()
    meta_logged = artifacts.artifact_metadata(fn + ":latest")
    assert meta_logged["Queried anime"] == query and meta_logged["content_weight"] == "rating"
    types = C.literal(rec["flags"]["SA_TYPES"])
    frame, frame_fn = C.content_similar_frame(anime_df, syn_df, query, 20, types=types)
    assert frame_fn == fn and got == frame.to_csv(index=False)
    assert len(frame) == 20 and query not in frame["Name"].tolist() and frame["Type"].isin(types).all()
    assert (np.diff(frame["Similarity"]) <= 0).all() and frame["Similarity"].iloc[0] > 0
    # the list from the restatement: the fit on the host, scores and select in NumPy
    meta = C.metadata_by_index(ids, anime_df, syn_df)
    vocab, off, ti, tw = R.tfidf({c: meta[c].tolist() for c in recs.CONTENT_COLUMNS})
    q = int(np.flatnonzero(ids == int(unrated["anime_id"].iloc[0]))[0])
    scores, err = R.content_scores(off, ti, tw, len(vocab), [0, 1], [q])
    own = np.zeros((1, len(ids)), bool)
    own[0, q] = True
    wi, wv = CR.rows_topk(scores, 20, keep=C.filter_mask(meta, anime_df, types).astype(np.uint8), wbits=CR.pack_bits(own))
    assert err == 0 and frame["Name"].tolist() == meta["Name"].to_numpy()[wi[0]].tolist()
    assert np.array_equal(_u32(frame["Similarity"].to_numpy(np.float32)), _u32(wv[0]))
    assert all(s for s in frame["Shared_tokens"][frame["Similarity"] > 0])
    # some listed titles have no rating either
    everything, _ = C.content_similar_frame(anime_df, syn_df, query, len(ids))
    assert len(everything) == len(ids) - 1 and set(unrated["Name"]) - {query} <= set(everything["Name"])


def test_content_recs_component_for_a_user(fixture_store):  # noqa: F811
    from anime_recommendations_amd import components as C, recs
    work, env, rec, df = (fixture_store[k] for k in ("work", "env", "rec", "df"))
    anime_df, syn_df = _fixture_frames(rec)
    user = int(rec["model_recs"]["cases"][0]["user"])
    _run("content_recs", _cr_flags(rec["flags"], user_query=user, content_weight="centered", content_min_rating=0.3,
                                   content_columns="Genres,Studios,Sypnopsis"), str(work), env)
    got = (work / ("User_ID_%d_content_recs.csv" % user)).read_text()
    cols = ["Genres", "Studios", "Sypnopsis"]
    frame = C.content_recs_frame(df, anime_df, syn_df, user, 20, columns=cols, weight="centered", min_rating=0.3)
    assert got == frame.to_csv(index=False) and len(frame) == 20
    mine = df[df.user_id == user]
    assert not set(frame["anime_id"]) & set(mine.anime_id) and (np.diff(frame["Content_score"]) <= 0).all()
    ids = C.content_universe(anime_df)
    meta = C.metadata_by_index(ids, anime_df, syn_df)
    vocab, off, ti, tw = R.tfidf({c: meta[c].tolist() for c in cols})
    assert {"Sypnopsis=synopsis", "Sypnopsis=anime", "Studios=Studio A", "Genres=Action"} <= set(vocab)
    pos = {a: i for i, a in enumerate(ids.tolist())}
    r = mine.rating.to_numpy().astype(np.float32)
    take = r >= np.float32(0.3)
    hist = [pos[a] for a in mine.anime_id.to_numpy()[take]]
    scores, err = R.content_scores(off, ti, tw, len(vocab), [0, len(hist)], hist, r[take] - r[take].mean(dtype=np.float32))
    seen = np.zeros((1, len(ids)), bool)
    seen[0, [pos[a] for a in mine.anime_id]] = True
    wi, wv = CR.rows_topk(scores, 20, keep=meta["has_meta"].to_numpy().astype(np.uint8), wbits=CR.pack_bits(seen))
    assert err == 0 and frame["anime_id"].tolist() == ids[wi[0]].tolist()
    assert np.array_equal(_u32(frame["Content_score"].to_numpy(np.float32)), _u32(wv[0]))
    code, out = _run_out("content_recs", _cr_flags(rec["flags"], user_query=user, anime_query="Naruto"), str(work), env)
    assert code != 0 and "exactly one" in out


def test_evaluate_baseline_content_on_the_recs_fixture(fixture_store):  # noqa: F811
    from anime_recommendations_amd import artifacts, components as C, data, recs, weights_io
    work, env, pq, rec = (fixture_store[k] for k in ("work", "env", "pq", "rec"))
    ks = [1, 5, 20]
    ev = dict(input_data="user_stats.parquet:latest", main_df_type="parquet", model="wandb_anime_nn.h5:latest",
              model_type="h5", project_name="anime_recommendations", test_size=1000, eval_k=str(ks), min_rating=0.7,
              eval_csv="content_metrics.csv", eval_type="eval_csv", ID_emb_name="user_embedding",
              anime_emb_name="anime_embedding")
    code, out = _run_out("evaluate", dict(ev, baseline="popularity,content", anime_df="all_anime.csv:latest",
                                          content_weight="centered", content_min_rating=0.2, ci_replicates=100),
                         str(work), env)
    assert code == 0, out[-3000:]
    summary = json.loads(out.strip().splitlines()[-1])
    frame = pd.read_csv(work / "content_metrics.csv", float_precision="round_trip")
    assert frame.columns.tolist()[:7] == ["k", "hit_rate", "ndcg", "hit_rate_popularity", "ndcg_popularity",
                                          "hit_rate_content", "ndcg_content"]
    assert {"hit_rate_diff_content", "hit_rate_p_content", "ndcg_content_lo", "ndcg_content_hi"} <= set(frame.columns)
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    table = data.load_user_stats(pq)
    pop_frame, pop = C.evaluate_frame(model, table, 1000, ks, 0.7, baseline="popularity", ci_replicates=100)
    assert frame[pop_frame.columns.tolist()].to_csv(index=False) == pop_frame.to_csv(index=False)
    assert {k: summary[k] for k in pop} == pop
    # the content figures from the restatement alone, on the training slice
    anime_df, _ = _fixture_frames(rec)
    meta = C.metadata_by_index(table.anime_ids, anime_df)
    vocab, off, ti, tw = R.tfidf({c: meta[c].tolist() for c in recs.CONTENT_COLUMNS})
    users, row, anime, train = recs.held_out_targets(table, 1000, 0.7)
    assert len(row) > 100
    tu, ta, tr = table.user[train], table.anime[train], table.rating[train].astype(np.float32)
    hoff, hist, hw = recs.history_csr(tu, ta, tr, users, 0.2)
    hw = recs.content_history_weights(hw, "centered", hoff)
    scores, err = R.content_scores(off, ti, tw, len(vocab), hoff, hist, hw)
    seen = np.zeros((len(users), table.n_anime), bool)
    for i, u in enumerate(users):
        seen[i, ta[tu == u]] = True
    rank, err2 = CR.rows_rank(scores, table.n_anime, table.n_anime, CR.pack_bits(seen), len(users), row, anime)
    assert err == 0 and err2 == 0
    b = recs.ranking_metrics(rank, ks)
    assert frame["hit_rate_content"].tolist() == [b["hit_rate"][k] for k in ks]
    assert frame["ndcg_content"].tolist() == [b["ndcg"][k] for k in ks]
    assert summary["content_mrr"] == b["mrr"] and summary["content_mean_rank"] == b["mean_rank"]
    code, out = _run_out("evaluate", dict(ev, baseline="content"), str(work), env)
    assert code != 0 and "--anime_df" in out


def test_hybrid_recs_takes_content_as_a_member(fixture_store):  # noqa: F811
    import torch
    from anime_recommendations_amd import artifacts, components as C, ops, recs, weights_io
    work, env, rec, df = (fixture_store[k] for k in ("work", "env", "rec", "df"))
    flags = rec["flags"]
    user = int(rec["model_recs"]["cases"][0]["user"])
    _run("hybrid_recs", dict(_mr_flags(flags, user, 15, "content.csv"), hybrid_systems="model,content"), str(work), env)
    got = (work / ("User_ID_%d_hybrid_content.csv" % user)).read_text()
    model = weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest", "h5"))
    anime_df, syn_df = _fixture_frames(rec)
    user_ids, anime_ids = C.index_tables(model, df)
    head = weights_io.model_head(model)
    frame, stats = C.hybrid_recs_frame(model["U"], model["A"], head, user_ids, anime_ids, df, anime_df, syn_df, user, 15,
                                       types=C.literal(flags["MR_TYPES"]), systems=("model", "content"))
    assert got == frame.to_csv(index=False) and stats["hybrid_systems"] == ["model", "content"]
    assert frame.columns.tolist()[-3:] == ["Hybrid_score", "Rank_model", "Rank_content"] and len(frame) == 15
    # the content member's ranks from the restatement, under the list's own mask
    meta = C.metadata_by_index(anime_ids, anime_df, syn_df)
    vocab, off, ti, tw = R.tfidf({c: meta[c].tolist() for c in recs.CONTENT_COLUMNS})
    ui, ai, r = C.rating_indices(df, user_ids, anime_ids)
    urow = int(np.flatnonzero(np.asarray(user_ids) == user)[0])
    hoff, hist, hr = recs.history_csr(ui, ai, r, [urow])
    scores, err = R.content_scores(off, ti, tw, len(vocab), hoff, hist, hr)
    blocked = ~C.filter_mask(meta, anime_df, C.literal(flags["MR_TYPES"])) | ~C.unwatched_mask(df, anime_ids, user)
    listed = np.asarray([int(np.flatnonzero(np.asarray(anime_ids) == a)[0]) for a in frame["anime_id"]])
    rank, err2 = CR.rows_rank(scores, len(anime_ids), len(anime_ids), CR.pack_bits(blocked[None]), 1,
                              np.zeros(len(listed), np.int64), listed)
    assert err == 0 and err2 == 0 and frame["Rank_content"].tolist() == (rank + 1).tolist()
