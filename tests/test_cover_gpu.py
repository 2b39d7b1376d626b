"""GPU tests of the onboarding lists (anirec_cover_greedy, anirec_cover_levels; ops.cover_greedy / cover_levels,
recs.onboarding_list, components.onboarding_frame and the onboarding component).

Yardstick: the NumPy restatement (tests/cover_restatement.py).  Every comparison is exact — picks, gains, info and levels
are integers; there is no tolerance anywhere.

Shapes: the smallest at which a kernel can go wrong — user counts around the 32-bit word, around the words a wave covers
per step of its row loop (anirec_cover_step_words: S) and past two steps with a tail (odd word counts, so rows that start
off a 16-byte boundary); item counts around the rows a workgroup holds at a time and past one workgroup."""
import ctypes

import numpy as np
import pytest

import cooc_restatement as CR
import cover_restatement as R
import poison
import recs_fixture as RF
from test_cooc_gpu import fixture_store  # noqa: F401  (the recs fixture as an artifact store)
from test_cover_cpu import host_ops, planted  # noqa: F401  (ops as the restatement, for the expected frames)
from test_recs_fixtures_gpu import _run

pytestmark = pytest.mark.gpu
N_ITEMS = (1, 2, 63, 64, 65, 130)
N_USERS = (1, 31, 32, 33, 70, "32S-1", "32S+1", "64S+163")


def _cuda(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _i32(b):
    return _cuda(np.ascontiguousarray(b).view(np.int32))


def _step():
    from anime_recommendations_amd import _lib
    return int(_lib.load().anirec_cover_step_words())


def _n_users(case):
    s = _step()
    return {"32S-1": 32 * s - 1, "32S+1": 32 * s + 1, "64S+163": 64 * s + 163}.get(case, case)


def _rated(n_items, n_users, density, seed):
    rng = np.random.default_rng(seed)
    M = rng.random((n_items, n_users)) < density
    if n_items >= 3:
        M[1] = False                                            # an item nobody rated
        M[-1] = M[0]                                            # twins: the lower index goes first
    return M


def _dirty(bits, n_users, seed):
    """garbage in the bits at positions >= n_users of every row's last word"""
    bits = bits.copy()
    tail = n_users % 32
    if tail:
        rng = np.random.default_rng(seed)
        bits[:, -1] |= (rng.integers(0, 1 << 32, len(bits), dtype=np.uint64).astype(np.uint32)
                        & np.uint32((0xFFFFFFFF << tail) & 0xFFFFFFFF))
    return bits


def _greedy(bits, n_users, m, depth, open_bits=None, keep=None):
    from anime_recommendations_amd import ops
    pick, gain, info = ops.cover_greedy(_i32(bits), n_users, m, depth, None if open_bits is None else _i32(open_bits),
                                        None if keep is None else _cuda(keep))
    return pick.cpu().numpy(), gain.cpu().numpy(), info.cpu().numpy()


def _same(got, want, what):
    for g, w, name in zip(got, want, ("pick", "gain", "info")):
        assert g.dtype == np.int32 and np.array_equal(g, w), (what, name, g.tolist(), w.tolist())


def _invariants(M, P, pick, gain, info, depth, what):
    made = int(info[0])
    assert (pick[:made] >= 0).all() and (pick[made:] == -1).all() and (gain[made:] == 0).all(), what
    assert len(set(pick[:made].tolist())) == made and (gain[:made] > 0).all(), what
    assert (np.diff(gain.astype(np.int64)) <= 0).all(), what
    held = M[pick[:made]].sum(axis=0) if made else np.zeros(M.shape[1], np.int64)
    assert int(gain.sum()) == int(np.minimum(depth, held)[P].sum()), what
    assert info.tolist() == [made, int((np.minimum(depth, held)[P] == depth).sum()), int(P.sum()), 0], what


# ---- cover_greedy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", N_ITEMS)
@pytest.mark.parametrize("users_case", N_USERS)
def test_cover_greedy_equals_the_restatement(users_case, n_items):
    n_users = _n_users(users_case)
    for density in (0.5, 0.02):
        M = _rated(n_items, n_users, density, 7 * n_items + n_users)
        clean = CR.pack_bits(M)
        bits = _dirty(clean, n_users, 3)
        rng = np.random.default_rng(n_items + n_users)
        P = rng.random(n_users) < 0.6
        open_bits = _dirty(CR.pack_bits(P[None]), n_users, 5)[0]
        keep = (rng.random(n_items) < 0.8).astype(np.uint8)
        everyone = np.ones(n_users, bool)
        for m, depth in ((1, 1), (n_items, 1), (min(n_items, 7), 2), (n_items + 3, 3), (min(n_items, 5), min(n_items, 5)),
                         (min(n_items, 9), 1000)):
            what = (users_case, n_items, density, m, depth)
            got = _greedy(bits, n_users, m, depth)
            _same(got, R.cover_greedy(clean, n_users, m, depth)[:3], what)
            _invariants(M, everyone, *got, depth, what)
            got = _greedy(bits, n_users, m, depth, open_bits, keep)
            _same(got, R.cover_greedy(clean, n_users, m, depth, open_bits, keep)[:3], what + ("open, keep",))
            _invariants(M, P, *got, depth, what)
            assert keep[got[0][got[0] >= 0]].all()


@pytest.mark.parametrize("side", (-1, 33))
def test_both_sides_of_the_lds_mask_switch(side):
    """the open mask is staged in LDS up to anirec_cover_lds_words() words and read from global memory past that"""
    from anime_recommendations_amd import _lib
    n_users, n_items = 32 * int(_lib.load().anirec_cover_lds_words()) + side, 19          # three workgroups' rows
    M = _rated(n_items, n_users, 0.05, 23 + side)
    clean = CR.pack_bits(M)
    bits = _dirty(clean, n_users, 3)
    P = np.random.default_rng(2).random(n_users) < 0.5
    open_bits = _dirty(CR.pack_bits(P[None]), n_users, 5)[0]
    for m, depth in ((n_items, 1), (6, 2), (5, 5)):
        got = _greedy(bits, n_users, m, depth, open_bits)
        _same(got, R.cover_greedy(clean, n_users, m, depth, open_bits)[:3], (side, m, depth))
        _invariants(M, P, *got, depth, (side, m, depth))


def test_edges_of_the_rule():
    from anime_recommendations_amd import ops
    n_items, n_users = 65, 32 * _step() + 1
    M = _rated(n_items, n_users, 0.3, 11)
    M[0, :] = True                                              # rows 0 and 64 hold everyone: the most popular, twins
    M[-1] = M[0]
    clean = CR.pack_bits(M)
    bits = _dirty(clean, n_users, 1)
    W = clean.shape[1]
    # twins: the lower index first; at depth 1 the twin then reaches nobody, at depth 2 it reaches everyone once more
    p1, g1, i1 = _greedy(bits, n_users, n_items, 1)
    assert p1.tolist() == [0] + [-1] * (n_items - 1) and g1[0] == n_users and i1.tolist() == [1, n_users, n_users, 0]
    p2, g2, i2 = _greedy(bits, n_users, 3, 2)
    assert p2.tolist()[:2] == [0, n_items - 1] and g2.tolist() == [n_users, n_users, 0] and p2[2] == -1
    assert i2.tolist() == [2, n_users, n_users, 0]
    _same((p2, g2, i2), R.cover_greedy(clean, n_users, 3, 2)[:3], "twins")
    # the empty row is never picked, with m = n_items the stop rule pads
    M2 = _rated(n_items, n_users, 0.02, 12)
    c2 = CR.pack_bits(M2)
    p, g, i = _greedy(_dirty(c2, n_users, 2), n_users, n_items, 3)
    _same((p, g, i), R.cover_greedy(c2, n_users, n_items, 3)[:3], "empty row")
    assert 1 not in p.tolist() and p[-1] == -1 and i[0] < n_items
    # an all-zero open_bits (garbage past n_users): no pick, info = {0, 0, 0, 0}
    nobody = _dirty(np.zeros((1, W), np.uint32), n_users, 9)[0]
    p, g, i = _greedy(bits, n_users, 4, 1, nobody)
    assert p.tolist() == [-1] * 4 and g.tolist() == [0] * 4 and i.tolist() == [0, 0, 0, 0]
    # one user in the population
    u = n_users - 2
    one = np.zeros(n_users, bool)
    one[u] = True
    p, g, i = _greedy(bits, n_users, 5, 2, CR.pack_bits(one[None])[0])
    rows = np.flatnonzero(M[:, u])
    assert p.tolist() == rows[:2].tolist() + [-1] * 3 and g.tolist() == [1, 1, 0, 0, 0] and i.tolist() == [2, 1, 1, 0]
    # a keep that removes the most popular row (and its twin); a keep of all zeros
    keep = np.ones(n_items, np.uint8)
    keep[0] = keep[-1] = 0
    got = _greedy(bits, n_users, 6, 2, None, keep)
    _same(got, R.cover_greedy(clean, n_users, 6, 2, None, keep)[:3], "keep")
    assert 0 not in got[0].tolist() and n_items - 1 not in got[0].tolist() and got[2][0] == 6
    p, g, i = _greedy(bits, n_users, 3, 1, None, np.zeros(n_items, np.uint8))
    assert p.tolist() == [-1] * 3 and g.tolist() == [0] * 3 and i.tolist() == [0, 0, n_users, 0]
    # depth = m without open_bits: a stable descending sort of the popcounts
    m = 20
    pop = ops.cooc_scores(_i32(bits), n_users, [0], pop=True)[3].cpu().numpy()
    order = np.argsort(-pop.astype(np.int64), kind="stable")[:m]
    p, g, i = _greedy(bits, n_users, m, m)
    assert p.tolist() == order.tolist() and g.tolist() == pop[order].tolist()
    for bad in (dict(m=0), dict(m=1025), dict(depth=0)):
        with pytest.raises(ValueError):
            ops.cover_greedy(_i32(bits), n_users, **dict(dict(m=3, depth=1), **bad))
    with pytest.raises(ValueError, match="open_bits"):
        ops.cover_greedy(_i32(bits), n_users, 3, 1, open_bits=_i32(np.zeros(W + 1, np.uint32)))
    with pytest.raises(ValueError, match="keep"):
        ops.cover_greedy(_i32(bits), n_users, 3, 1, keep=_cuda(np.ones(n_items + 1, np.uint8)))


# ---- independence -----------------------------------------------------------------------------------------------------
def _case_a():
    n_items, n_users = 130, 64 * _step() + 163
    M = _rated(n_items, n_users, 0.1, 31)
    P = np.random.default_rng(1).random(n_users) < 0.5
    return M, _dirty(CR.pack_bits(M), n_users, 4), n_users, _dirty(CR.pack_bits(P[None]), n_users, 6)[0]


def test_a_call_alone_and_after_a_call_of_another_shape():
    from anime_recommendations_amd import ops
    M, bits, n_users, open_bits = _case_a()
    want = R.cover_greedy(CR.pack_bits(M), n_users, 40, 2, open_bits)[:3]
    ops.release_workspaces()
    _same(_greedy(bits, n_users, 40, 2, open_bits), want, "alone")
    assert len(ops._COVER_WS) == 1
    ws = next(iter(ops._COVER_WS.values()))
    other = _rated(300, 8 * _step() + 77, 0.5, 5)              # more rows, fewer users: another layout of the same bytes
    ob = CR.pack_bits(other)
    _same(_greedy(ob, other.shape[1], 64, 64), R.cover_greedy(ob, other.shape[1], 64, 64)[:3], "the other shape")
    assert next(iter(ops._COVER_WS.values())) is ws             # the same cached workspace
    _same(_greedy(bits, n_users, 40, 2, open_bits), want, "after another shape")
    _same(_greedy(bits, n_users, 40, 2, open_bits), want, "after itself")


@pytest.mark.parametrize("byte", poison.ORDER)
def test_cover_ignores_what_its_buffers_held(byte):
    from anime_recommendations_amd import ops
    M, bits, n_users, open_bits = _case_a()
    b, ob = _i32(bits), _i32(open_bits)
    ops.release_workspaces()                                    # so the workspace is handed out dirty too
    log = []
    with poison.poisoned(byte, log):
        pick, gain, info = ops.cover_greedy(b, n_users, 12, 2, ob)
        level = ops.cover_levels(b, n_users, pick)
    assert len(log) >= 5 and max(log) >= n_users // 8           # the outputs, the workspace, the levels
    want = R.cover_greedy(CR.pack_bits(M), n_users, 12, 2, open_bits)
    _same((pick.cpu().numpy(), gain.cpu().numpy(), info.cpu().numpy()), want[:3], byte)
    assert np.array_equal(level.cpu().numpy(), R.cover_levels(CR.pack_bits(M), n_users, want[0])[0])


def test_cover_greedy_replays_from_a_graph():
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    M, bits, n_users, open_bits = _case_a()
    n_items, m, depth = M.shape[0], 24, 2
    b, ob = _i32(bits), _i32(open_bits)
    pick, gain = [poison.fill(torch.empty(m, dtype=torch.int32, device="cuda"), 0x3F) for _ in range(2)]
    info = poison.fill(torch.empty(4, dtype=torch.int32, device="cuda"), 0x3F)
    ws = poison.fill(torch.empty(int(lib.anirec_cover_workspace_bytes(n_items, n_users)), dtype=torch.uint8,
                                 device="cuda"), 0x7F)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st = lib.anirec_cover_greedy(_lib.ptr(b), n_items, n_users, _lib.ptr(ob), None, depth, m, _lib.ptr(pick),
                                     _lib.ptr(gain), _lib.ptr(info), _lib.ptr(ws), ws.numel(), s)
    assert st == 0
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0x3F).all()) for t in (pick, gain, info))      # captured, not run
    eager = _greedy(bits, n_users, m, depth, open_bits)
    _same(eager, R.cover_greedy(CR.pack_bits(M), n_users, m, depth, open_bits)[:3], "eager")
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _same((pick.cpu().numpy(), gain.cpu().numpy(), info.cpu().numpy()), eager, "replay")
        for t in (pick, gain, info):
            poison.fill(t, 0x7F)


# ---- cover_levels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("users_case", (1, 33, "32S+1"))
def test_cover_levels(users_case):
    from anime_recommendations_amd import ops
    n_users, n_items = _n_users(users_case), 65
    M = _rated(n_items, n_users, 0.3, 17)
    clean = CR.pack_bits(M)
    b = _i32(_dirty(clean, n_users, 8))
    picks = np.array([3, -1, 64, 3, 0, -1, 1], np.int32)         # padding, a repeat, the empty row
    level = ops.cover_levels(b, n_users, picks).cpu().numpy()
    assert level.dtype == np.int32 and np.array_equal(level, M[[3, 64, 3, 0, 1]].sum(axis=0))
    assert np.array_equal(level, R.cover_levels(clean, n_users, picks)[0])
    for bad in (n_items, -2, 2 ** 31 - 1):
        with pytest.raises(ValueError, match="out of range"):
            ops.cover_levels(b, n_users, list(picks) + [bad])
        lv, err = ops.cover_levels(b, n_users, list(picks) + [bad], check=False)
        assert int(err.item()) == 1 and np.array_equal(lv.cpu().numpy(), level)       # the other counts intact
    assert ops.cover_levels(b, n_users, np.zeros(0, np.int32)).cpu().numpy().tolist() == [0] * n_users
    pick, gain, info = ops.cover_greedy(b, n_users, n_items, 2)             # its own out_pick, padding included
    assert int(info[0]) < n_items
    lv = ops.cover_levels(b, n_users, pick).cpu().numpy()
    assert np.array_equal(lv, R.cover_levels(clean, n_users, pick.cpu().numpy())[0])
    assert int(np.minimum(lv, 2).sum()) == int(gain.sum()) and int((lv >= 2).sum()) == int(info[1])


# ---- the planted case, the recs layer and the component ---------------------------------------------------------------
def test_planted_case_on_the_device(request):
    from anime_recommendations_amd import recs
    M = planted()
    bits = CR.pack_bits(M)
    assert [x.tolist() for x in _greedy(bits, 16, 2, 1)] == [[0, 2], [10, 6], [2, 16, 16, 0]]
    assert [x.tolist() for x in _greedy(bits, 16, 2, 2)] == [[0, 1], [10, 9], [2, 9, 16, 0]]
    a, u = np.nonzero(M)
    settings = [dict(depth=1), dict(depth=2), dict(depth=1, strategy="popularity"),
                dict(depth=1, holdout=0.25, seed=3), dict(depth=1, population=np.arange(10, 16), m=3),
                dict(depth=1, keep=[0, 1, 1])]
    got = [recs.onboarding_list(u, a, 16, 3, **dict(dict(m=2), **kw)) for kw in settings]
    request.getfixturevalue("host_ops")                          # from here on ops is the restatement
    for kw, g in zip(settings, got):
        w = recs.onboarding_list(u, a, 16, 3, **dict(dict(m=2), **kw))
        assert sorted(g) == sorted(w)
        for key in w:
            assert np.array_equal(g[key], w[key]) if isinstance(w[key], np.ndarray) else g[key] == w[key], (kw, key)
    assert got[0]["pick"].tolist() == [0, 2] and got[2]["pick"].tolist() == [0, 1]
    assert got[0]["pick_users"]["share_any"] == 1.0 and got[2]["pick_users"]["share_any"] == 10 / 16


def test_onboarding_component_on_the_recs_fixture(fixture_store, request):
    from anime_recommendations_amd import artifacts, components as C
    work, env, rec, df = (fixture_store[k] for k in ("work", "env", "rec", "df"))
    flags = rec["flags"]
    fn = "onboarding_list.csv"
    ob = dict(project_name="anime_recommendations", main_df="user_stats.parquet:latest", main_df_type="parquet",
              anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopses_df="synopses.csv:latest",
              sypnopsis_df_type="raw_data", anime_rec_genres=flags["SA_GENRES"], an_spec_genres=False,
              types=flags["SA_TYPES"], spec_types=True, onboard_fn=fn, onboard_type="csv", save_onboard=True,
              onboard_number=12, onboard_depth=6, onboard_strategy="coverage", onboard_max_ratings=412,
              onboard_holdout=0.3, onboard_seed=4)
    _run("onboarding", ob, str(work), env)
    got = (work / fn).read_text()
    meta = artifacts.artifact_metadata(fn + ":latest")
    anime_df = C.load_anime_df(RF.csv(rec, "anime_csv"))
    syn_df = C.load_synopses(RF.csv(rec, "synopses_csv"))
    kw = dict(types=C.literal(flags["SA_TYPES"]), max_ratings=412, holdout=0.3, seed=4)
    gpu_frame, gpu_summary = C.onboarding_frame(df, anime_df, syn_df, 12, 6, "coverage", **kw)
    assert got == gpu_frame.to_csv(index=False)
    request.getfixturevalue("host_ops")                          # from here on ops is the restatement
    want, summary = C.onboarding_frame(df, anime_df, syn_df, 12, 6, "coverage", **kw)
    assert got == want.to_csv(index=False) and gpu_summary == summary
    assert {k: meta[k] for k in summary} == summary and meta["Filename"] == fn
    assert 0 < len(want) <= 12 and want["Type"].isin(C.literal(flags["SA_TYPES"])).all()
    assert (np.diff(want["New_reach"]) <= 0).all() and 0 < summary["population"]
    assert summary["coverage"]["holdout_users"]["users"] == summary["popularity"]["holdout_users"]["users"] > 0
