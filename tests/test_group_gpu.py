"""GPU tests of group recommendations (anirec_group_topk, ops.group_topk, recs.group_topk, the group_recs component).

Yardstick: the NumPy restatement (tests/group_restatement.py) run on the grid the existing ``ops.predict_grid`` returns
for the same tables — that kernel is not under test here, and the header defines a member's rating as its bits.  Every
idx, every score and every member rating is compared bit for bit.

Shapes: 333 anime (five 64-tiles and a 13-row tail; eleven mask words, the last with 13 bits), 50 users, widths 32, 64,
128 and 256; 37 groups a call of sizes 1, 2, 3, 4, 5, 63 and 64 (so that m_pad = next_pow2(max_members) is 64) and calls
whose largest group has 1, 2, 4 and 5 members (m_pad 1, 2, 4, 8); k 1, 10, 128, 129, 333 and 400 (both selects, the whole
ranking, k > n).  The ranking of a group does not depend on k, so the reference is computed once per (width, head,
mode, floor) for k = 400 and its first columns are the reference for every smaller k.
"""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

import group_restatement as G
import poison
from rank_restatement import pack
from test_components_gpu import _run, pipeline  # noqa: F401  (the components' pipeline fixture, as it is)

pytestmark = pytest.mark.gpu
N_A, N_U, N_G, K_ALL = 333, 50, 37, 400
WORDS = (N_A + 31) // 32
WIDTHS = (32, 64, 128, 256)
KS = (1, 10, 128, 129, 333, 400)
TWIN_A, TWIN_B = 40, 200                   # two bit-identical anime rows: every rating ties, every aggregate ties
NAN_POS, ALL_POS, SOLO_POS = 6, 11, 5      # positions in USERS: a row holding a NaN, a member who has watched everything
HEAD = dict(w=1.3, b=-0.1, gamma=0.9, beta=0.05, mov_mean=0.02, mov_var=0.8)
USERS = np.random.default_rng(77).permutation(N_U)      # positions are not row numbers
MODE_NAMES = {"mean": "mean", "min": "least_misery", "max": "most_pleasure"}


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_TABLES = {}


def _tables(dim, act="sigmoid"):
    """(U, A on the device, head, P [N_U, N_A]: row i = ops.predict_grid's ratings of user USERS[i]), once per kind"""
    if (dim, act) not in _TABLES:
        from anime_recommendations_amd import ops
        rng = np.random.default_rng(200 + dim)
        U = rng.normal(size=(N_U, dim)).astype(np.float32)
        A = rng.normal(size=(N_A, dim)).astype(np.float32)
        A[TWIN_B] = A[TWIN_A]
        U[USERS[NAN_POS], 3] = np.nan
        head = dict(HEAD, activation=act)
        tU, tA = _cuda(U), _cuda(A)
        P = ops.predict_grid(tU, tA, head, USERS).cpu().numpy()
        assert not np.isnan(np.delete(P, NAN_POS, axis=0)).any()
        assert (P[NAN_POS] == 0).all() if act == "relu" else np.isnan(P[NAN_POS]).all()       # (fmaxf(NaN, 0) is 0)
        assert np.array_equal(_bits(P[:, TWIN_A]), _bits(P[:, TWIN_B]))
        _TABLES[(dim, act)] = (tU, tA, head, P)
    return _TABLES[(dim, act)]


def _groups():
    """the 37 groups of a call as lists of positions in USERS: the planted ones first, then sizes 1 .. 5, 63, 64 in turn"""
    rng = np.random.default_rng(9)
    plain = [p for p in range(N_U) if p not in (NAN_POS, ALL_POS)]
    groups = [[NAN_POS, 1, 2],                  # 0: a member whose ratings are NaN
              [7, 7],                           # 1: a repeated member
              [],                               # 2: an empty group
              [ALL_POS, 4],                     # 3: a member who has watched everything: no candidates
              [SOLO_POS], [SOLO_POS] * 2, [SOLO_POS] * 4,       # 4, 5, 6: one user alone, twice, four times
              [3, 8], [8, 9, 10],               # 7, 8: user 8 in two groups
              [1, NAN_POS]]                     # 9: the NaN member last
    sizes = (1, 2, 3, 4, 5, 63, 64)
    while len(groups) < N_G:
        groups.append(rng.choice(plain, sizes[len(groups) % len(sizes)]).tolist())
    assert sorted({len(g) for g in groups}) == [0, 1, 2, 3, 4, 5, 63, 64]
    return groups


def _csr(groups):
    offsets = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=offsets[1:])
    return offsets, np.asarray([p for g in groups for p in g], np.int32)


def _masks():
    """(watched bool [N_U, N_A], exclude bool [N_G, N_A], and their bit words; the watched words carry random bits past
    N_A in the last word, which must have no effect)"""
    rng = np.random.default_rng(4)
    watched = rng.random((N_U, N_A)) < 0.02                     # light watchers: a 64-member group keeps candidates
    watched[[3, SOLO_POS, 7, 8]] = rng.random((4, N_A)) < 0.3   # and four heavy ones
    watched[ALL_POS] = True
    watched[SOLO_POS, [TWIN_A, TWIN_B]] = False
    exclude = rng.random((N_G, N_A)) < 0.1
    exclude[4:7, [TWIN_A, TWIN_B]] = False
    exclude[12] = True                                          # a group whose exclude row leaves nothing
    wbits = pack(watched)
    wbits[:, -1] |= rng.integers(0, 1 << 32, N_U, dtype=np.uint64).astype(np.uint32) & ~np.uint32((1 << (N_A % 32)) - 1)
    assert wbits.shape == (N_U, WORDS) and (wbits[:, -1] >> np.uint32(N_A % 32)).any()
    return watched, exclude, wbits.view(np.int32), pack(exclude).view(np.int32)


def _floor(P):
    """a rating of the grid: above it for every member of a small group often, of a 63-member group hardly ever"""
    vals = np.sort(P[~np.isnan(P)])
    return np.float32(vals[int(0.6 * len(vals))])


_REFS = {}


def _reference(dim, act, mode, with_floor):
    key = (dim, act, mode, with_floor)
    if key not in _REFS:
        P = _tables(dim, act)[3]
        offsets, member_row = _csr(_groups())
        watched, exclude, _, _ = _masks()
        _REFS[key] = G.group_topk(P, offsets, member_row, K_ALL, mode, _floor(P) if with_floor else None, watched, exclude)
    return _REFS[key]


def _same(got, ref, k, what):
    gi, gs, gm = [t.cpu().numpy() for t in got]
    assert np.array_equal(gi, ref[0][:, :k]), what
    assert np.array_equal(_bits(gs), _bits(ref[1][:, :k])), what
    assert np.array_equal(_bits(gm), _bits(ref[2][:, :k])), what


def _call(dim, act, mode, with_floor, k, groups=None, **kw):
    from anime_recommendations_amd import ops
    tU, tA, head, P = _tables(dim, act)
    offsets, member_row = _csr(_groups() if groups is None else groups)
    _, _, wbits, xbits = _masks()
    kw.setdefault("exclude_bits", xbits if groups is None else None)
    return ops.group_topk(tU, tA, head, USERS, offsets, member_row, k, mode=MODE_NAMES[mode],
                          floor=_floor(P) if with_floor else None, watched_bits=wbits, member_ratings=True, **kw)


@pytest.mark.parametrize("with_floor", [False, True])
@pytest.mark.parametrize("mode", G.MODES)
@pytest.mark.parametrize("dim", WIDTHS)
def test_group_topk_equals_the_restatement(dim, mode, with_floor):
    ref = _reference(dim, "sigmoid", mode, with_floor)
    for k in KS:
        _same(_call(dim, "sigmoid", mode, with_floor, k), ref, k, (dim, mode, with_floor, k))
    # the planted content did what it is there for (checked on the reference, which the kernel has just equalled)
    ri, rs, rm = ref
    n_cand = (ri >= 0).sum(axis=1)
    assert n_cand[2] == 0 and n_cand[3] == 0 and n_cand[12] == 0 and np.isnan(rs[[2, 3, 12]]).all()
    assert (ri[:, N_A:] == -1).all() and n_cand.max() < N_A
    offsets, _ = _csr(_groups())
    assert np.isnan(rm[offsets[3]:offsets[4]]).all()
    if with_floor:
        print("candidates left under the floor: fewest %d, most %d" % (n_cand.min(), n_cand.max()))
        assert ((n_cand > 0) & (n_cand < 10)).any() and (n_cand > 10).any()
    else:
        row = ri[4].tolist()                                    # the twins tie: the lower index first, next to each other
        assert row.index(TWIN_B) == row.index(TWIN_A) + 1
        assert n_cand[0] > 10 and np.isnan(rm[offsets[0], :n_cand[0]]).all()      # the NaN member's own ratings
        if mode == "mean":
            assert np.isnan(rs[0, :n_cand[0]]).all() and ri[0, :n_cand[0]].tolist() == sorted(ri[0, :n_cand[0]].tolist())
        else:                                                   # MIN / MAX keep the NaN whichever member brings it
            assert np.isnan(rs[[0, 9], :5]).all()


@pytest.mark.parametrize("act", ["linear", "tanh", "relu", "softplus"])
def test_other_activations(act):
    for mode in G.MODES:
        ref = _reference(64, act, mode, False)
        for k in (10, 333):
            _same(_call(64, act, mode, False, k), ref, k, (act, mode, k))
    if act == "relu":                                           # whole runs of ties at 0: ascending index
        ri, rs, _ = _reference(64, act, "min", False)
        zero = rs[7] == 0
        assert zero.sum() > 20 and (np.diff(ri[7][zero]) > 0).all()


@pytest.mark.parametrize("biggest", [1, 2, 4, 5])
def test_smaller_tiles(biggest):
    """calls whose largest group has 1, 2, 4 and 5 members: 64, 32, 16 and 8 groups a tile"""
    groups = [g for g in _groups() if len(g) <= biggest]
    groups = groups * ((64 // biggest) // len(groups) + 2)      # more groups than one tile holds
    assert max(len(g) for g in groups) == biggest and len(groups) > 64 // biggest
    dim, mode = 128, "mean"
    P = _tables(dim)[3]
    offsets, member_row = _csr(groups)
    watched = _masks()[0]
    for k in (10, 200):
        ref = G.group_topk(P, offsets, member_row, k, mode, None, watched, None)
        _same(_call(dim, "sigmoid", mode, False, k, groups=groups), ref, k, (biggest, k))


def test_a_single_group_of_four():
    groups = [[20, 21, 22, 23]]
    P = _tables(128)[3]
    offsets, member_row = _csr(groups)
    for mode in G.MODES:
        for k in (10, 333):
            ref = G.group_topk(P, offsets, member_row, k, mode, None, _masks()[0], None)
            _same(_call(128, "sigmoid", mode, False, k, groups=groups), ref, k, (mode, k))


@pytest.mark.parametrize("dim", WIDTHS)
def test_one_member_group_is_predict_topk(dim):
    """in all three modes, for both selects; [u, u] and [u, u, u, u] under MEAN are u's own list as well"""
    import torch
    from anime_recommendations_amd import ops
    tU, tA, head, _ = _tables(dim)
    wbits = _masks()[2]
    solo = [[p] for p in (SOLO_POS, NAN_POS, ALL_POS, 30)]
    for k in (10, 200):
        wi, wp = ops.predict_topk(tU, tA, head, USERS[[g[0] for g in solo]], k, wbits[[g[0] for g in solo]])
        for mode in G.MODES:
            gi, gs, gm = _call(dim, "sigmoid", mode, False, k, groups=solo)
            assert torch.equal(gi, wi) and torch.equal(gs.view(torch.int32), wp.view(torch.int32)), (mode, k)
            assert torch.equal(gm.view(torch.int32), wp.view(torch.int32))
        for copies in (2, 4):
            gi, gs, gm = _call(dim, "sigmoid", "mean", False, k, groups=[g * copies for g in solo])
            assert torch.equal(gi, wi) and torch.equal(gs.view(torch.int32), wp.view(torch.int32)), (copies, k)


# ---- the entry point itself -------------------------------------------------------------------------------------
def _raw(dim=128, k=10, mode=0, groups=None, offsets=None, member_row=None, max_members=None, ws_bytes=None, floor=None,
         null=None, fill=0x3F, n_members=None, **scalars):
    """anirec_group_topk itself on the call of the main test, its outputs and flag pre-filled with ``fill`` bytes: no
    wrapper check between the test and the entry point.  ``null``: the name of one pointer passed as NULL; ``scalars``:
    dim_arg / n_anime / n_users / act / n_groups values that replace the true ones.  Returns (status, outs, err)."""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    tU, tA, head, _ = _tables(dim)
    go, gm = _csr(_groups() if groups is None else groups)
    offsets = go if offsets is None else np.asarray(offsets, np.int32)
    member_row = gm if member_row is None else np.asarray(member_row, np.int32)
    n_g, n_m = len(offsets) - 1, len(member_row) if n_members is None else n_members
    if max_members is None:
        max_members = max(1, int(np.diff(go).max()))
    _, _, wbits, xbits = _masks()
    kk = max(k, 1)
    outs = [poison.fill(torch.empty((n_g, kk), dtype=torch.int32, device="cuda"), fill),
            poison.fill(torch.empty((n_g, kk), dtype=torch.float32, device="cuda"), fill),
            poison.fill(torch.empty((max(len(member_row), 1), kk), dtype=torch.float32, device="cuda"), fill)]
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), fill)
    full = int(lib.anirec_group_topk_workspace_bytes(N_A, N_U, n_g, kk, dim))
    ws = poison.fill(torch.empty(full, dtype=torch.uint8, device="cuda"), fill)
    p = dict(U=tU, A=tA, users=_cuda(USERS.astype(np.int32)), watched=_cuda(wbits), offsets=_cuda(offsets),
             member_row=_cuda(member_row), exclude=_cuda(xbits) if groups is None else None, out_idx=outs[0],
             out_score=outs[1], out_member_p=outs[2], err=err, ws=ws)
    if null and null != "head":
        p[null] = None
    h = _lib.Head(*[float(head[f]) for f in ("w", "b", "gamma", "beta", "mov_mean", "mov_var")])
    s = dict(dim=dim, n_anime=N_A, n_users=N_U, act=0, n_groups=n_g)
    s.update({("dim" if name == "dim_arg" else name): v for name, v in scalars.items()})
    st = lib.anirec_group_topk(_lib.ptr(p["U"]), _lib.ptr(p["A"]), s["dim"], s["n_anime"], _lib.ptr(p["users"]),
                               s["n_users"], None if null == "head" else ctypes.byref(h), s["act"], _lib.ptr(p["watched"]),
                               _lib.ptr(p["offsets"]), _lib.ptr(p["member_row"]), s["n_groups"], n_m, max_members,
                               _lib.ptr(p["exclude"]), mode, float("-inf") if floor is None else floor, k,
                               _lib.ptr(p["out_idx"]), _lib.ptr(p["out_score"]), _lib.ptr(p["out_member_p"]),
                               _lib.ptr(p["err"]), _lib.ptr(p["ws"]), full if ws_bytes is None else ws_bytes,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, outs, err


def test_a_group_does_not_depend_on_its_context():
    """a group run alone, at another position among other groups, with max_members 4 and 64, with the smallest
    workspace (one group a batch) and the full one, and twice: the same bits"""
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    dim, mode = 128, "min"
    ref = _reference(dim, "sigmoid", mode, False)
    offsets, _ = _csr(_groups())
    groups = _groups()
    for k in (10, 200):
        st, outs, err = _raw(dim, k, 1)
        assert st == 0 and int(err.item()) == 0
        _same(outs, ref, k, "whole call")
        one_group = int(lib.anirec_group_topk_workspace_bytes(N_A, N_U, 1, k, dim))
        assert one_group < int(lib.anirec_group_topk_workspace_bytes(N_A, N_U, N_G, k, dim))
        st, outs, err = _raw(dim, k, 1, ws_bytes=one_group)
        assert st == 0
        _same(outs, ref, k, "one group a batch")
        assert _raw(dim, k, 1, ws_bytes=one_group - 1)[0] == -3
        share = int(lib.anirec_group_topk_workspace_bytes(N_A, N_U, 2, k, dim)) - one_group
        assert 0 < share and one_group + 4 * share < int(lib.anirec_group_topk_workspace_bytes(N_A, N_U, N_G, k, dim))
        st, outs, err = _raw(dim, k, 1, ws_bytes=one_group + 4 * share + 5)     # five groups a batch
        assert st == 0
        _same(outs, ref, k, "a few groups a batch")
    k = 10
    perm = np.random.default_rng(5).permutation(N_G)
    moved = _call(dim, "sigmoid", mode, False, k, groups=[groups[g] for g in perm], exclude_bits=_masks()[3][perm])
    ends = np.concatenate([np.arange(offsets[g], offsets[g + 1]) for g in perm]).astype(np.int64)
    _same(moved, (ref[0][perm], ref[1][perm], ref[2][ends]), k, "permuted call")
    small = [g for g in range(N_G) if 0 < len(groups[g]) <= 4]
    for g in small[:6]:
        want = (ref[0][g:g + 1], ref[1][g:g + 1], ref[2][offsets[g]:offsets[g + 1]])
        for max_members in (4, 64):
            st, outs, err = _raw(dim, k, 1, groups=[groups[g]], max_members=max_members)
            assert st == 0 and int(err.item()) == 0
            # (no exclude row in a call with its own groups: compare against the restatement without one)
            alone = G.group_topk(_tables(dim)[3], *_csr([groups[g]]), k, mode, None, _masks()[0], None)
            _same(outs, alone, k, (g, max_members))
        alone_x = _call(dim, "sigmoid", mode, False, k, groups=[groups[g]], exclude_bits=_masks()[3][g:g + 1])
        _same(alone_x, want, k, "group %d alone" % g)


@pytest.mark.parametrize("byte", poison.ORDER)
def test_dirty_memory_changes_nothing(byte):
    for dim, mode, k in ((32, "mean", 10), (128, "max", 200)):
        log = []
        with poison.poisoned(byte, log):
            got = _call(dim, "sigmoid", mode, True, k)
        assert len(log) == 5                                    # idx, score, member_p, the flag word, the workspace
        _same(got, _reference(dim, "sigmoid", mode, True), k, (byte, dim))


def _poisoned_ref(ref, groups_bad, offsets):
    ri, rs, rm = [r.copy() for r in ref]
    for g in groups_bad:
        ri[g], rs[g] = -1, np.nan
        rm[offsets[g]:offsets[g + 1]] = np.nan
    return ri, rs, rm


@pytest.mark.parametrize("bad_value", [-1, N_U, 2 ** 31 - 1])
def test_a_bad_member_row_poisons_its_own_group_alone(bad_value):
    dim, mode, k = 64, "mean", 10
    offsets, member_row = _csr(_groups())
    ref = _reference(dim, "sigmoid", mode, False)
    for g in (8, 26):                                           # a 3-member group, and a big one
        assert offsets[g + 1] - offsets[g] >= 3
        bad = member_row.copy()
        bad[offsets[g + 1] - 1] = bad_value
        st, outs, err = _raw(dim, k, 0, member_row=bad)
        assert st == 0 and int(err.item()) == 1
        _same(outs, _poisoned_ref(ref, [g], offsets), k, (bad_value, g))
    st, outs, err = _raw(dim, k, 0)                             # and the flag is cleared by a clean call
    assert st == 0 and int(err.item()) == 0
    _same(outs, ref, k, "clean")


def test_bad_offsets_poison_their_own_groups_alone():
    dim, mode, k = 64, "mean", 10
    groups = _groups()
    offsets, member_row = _csr(groups)
    ref = _reference(dim, "sigmoid", mode, False)
    assert len(groups[0]) == 3 and len(groups[N_G - 1]) > 0
    # a decreasing pair (group 0 becomes (4, 3): its members are in no valid group any more), a negative start, and an
    # end past n_members (the last group's)
    for g, lo_hi in ((0, (4, None)), (0, (-2, None)), (N_G - 1, (None, len(member_row) + 1))):
        off = offsets.copy()
        if lo_hi[0] is not None:
            off[g] = lo_hi[0]
        if lo_hi[1] is not None:
            off[g + 1] = lo_hi[1]
        st, outs, err = _raw(dim, k, 0, offsets=off)
        assert st == 0 and int(err.item()) == 1
        _same(outs, _poisoned_ref(ref, [g], offsets), k, (g, lo_hi))


def test_a_group_above_the_cap():
    from anime_recommendations_amd import ops
    tU, tA, head, _ = _tables(64)
    groups = [[1, 2, 3], list(range(40)) + list(range(25)), [4, 5]]           # 65 members in the middle
    offsets, member_row = _csr(groups)
    with pytest.raises(ValueError, match="65 members is above the limit of 64"):
        ops.group_topk(tU, tA, head, USERS, offsets, member_row, 10)
    assert _raw(64, 10, 0, groups=groups, max_members=65)[0] == -1            # the entry point refuses the bound itself
    st, outs, err = _raw(64, 10, 0, groups=groups, max_members=64)            # and a group above the bound it was given
    assert st == 0 and int(err.item()) == 1
    ref = G.group_topk(_tables(64)[3], offsets, member_row, 10, "mean", None, _masks()[0], None)
    _same(outs, _poisoned_ref(ref, [1], offsets), 10, "65 members")
    with pytest.raises(ValueError, match="out of range"):                     # the wrapper raises on the flag
        ops.group_topk(tU, tA, head, USERS, [0, 2], [0, N_U], 10)


def test_einval_returns_before_writing():
    import torch
    cases = [dict(dim_arg=48), dict(dim_arg=0), dict(act=5), dict(act=-1), dict(mode=3), dict(mode=-1), dict(floor=float("nan")),
             dict(n_anime=0), dict(n_users=-1), dict(n_groups=-1), dict(n_members=-1), dict(k=0), dict(max_members=0),
             dict(max_members=65)]
    cases += [dict(null=n) for n in ("U", "A", "users", "head", "offsets", "member_row", "out_idx", "out_score", "err", "ws")]

    def untouched(tensors):
        return all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in tensors)

    for kw in cases:
        st, outs, err = _raw(**kw)
        assert st == -1 and untouched(outs + [err]), kw
    st, outs, err = _raw(n_groups=0)                            # no groups: ok, nothing enqueued
    assert st == 0 and untouched(outs + [err])
    for null in ("watched", "exclude", "out_member_p"):         # the optional ones
        st, outs, err = _raw(null=null)
        assert st == 0 and int(err.item()) == 0 and (null != "out_member_p" or untouched(outs[2:]))


def test_the_call_is_graph_capturable():
    """captured into a graph the call runs nothing; the replay writes the restatement's bits and clears the flag"""
    import torch
    from anime_recommendations_amd import _lib
    lib = _lib.load()
    dim, k = 128, 10
    tU, tA, head, _ = _tables(dim)
    offsets, member_row = _csr(_groups())
    _, _, wbits, xbits = _masks()
    outs = [poison.fill(torch.empty((N_G, k), dtype=torch.int32, device="cuda"), 0x3F),
            poison.fill(torch.empty((N_G, k), dtype=torch.float32, device="cuda"), 0x3F),
            poison.fill(torch.empty((len(member_row), k), dtype=torch.float32, device="cuda"), 0x3F)]
    err = poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), 0x3F)
    ws = torch.empty(int(lib.anirec_group_topk_workspace_bytes(N_A, N_U, N_G, k, dim)), dtype=torch.uint8, device="cuda")
    dev = [_cuda(x) for x in (USERS.astype(np.int32), wbits, offsets, member_row, xbits)]
    h = _lib.Head(*[float(head[f]) for f in ("w", "b", "gamma", "beta", "mov_mean", "mov_var")])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = lib.anirec_group_topk(_lib.ptr(tU), _lib.ptr(tA), dim, N_A, _lib.ptr(dev[0]), N_U, ctypes.byref(h), 0,
                                   _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), N_G, len(member_row), 64,
                                   _lib.ptr(dev[4]), 0, float("-inf"), k, *[_lib.ptr(o) for o in outs], _lib.ptr(err),
                                   _lib.ptr(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    assert all(bool((t.view(-1).view(torch.uint8) == 0x3F).all()) for t in outs + [err])     # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    _same(outs, _reference(dim, "sigmoid", "mean", False), k, "graph replay")


# ---- recs.group_topk and the component, on the pipeline of test_components_gpu.py -------------------------------
def _model():
    from anime_recommendations_amd import artifacts, weights_io
    return weights_io.load_model(artifacts.use_artifact("wandb_anime_nn.h5:latest"))


def _flags(user, **extra):
    return dict(main_df="user_stats.parquet:latest", main_df_type="parquet", project_name="anime_recommendations",
                anime_df="all_anime.csv:latest", anime_df_type="raw_data", sypnopsis_df="synopses.csv:latest",
                sypnopsis_df_type="raw_data", model="wandb_anime_nn.h5:latest", model_type="h5",
                model_user_query=user, random_user=False, model_recs_fn="model_recs.csv", save_model_recs=True,
                model_num_recs=10, anime_types='["TV", "Movie"]', specify_types=True,
                model_genres='["Action", "Comedy", None]', specify_genres=False, model_ID_flow=False,
                model_ID_conf=True, model_recs_type="csv", flow_ID="user_id.csv:latest", flow_ID_type="csv", **extra)


def test_recs_group_topk_on_the_trained_model(pipeline):  # noqa: F811
    from anime_recommendations_amd import ops, recs
    m = _model()
    uid = np.asarray(m["user_ids"])
    groups = [[int(uid[3]), int(uid[50])], [int(uid[50])], [int(uid[7]), int(uid[3]), int(uid[7])]]
    gi, gs, gm, (users, offsets, member_row) = recs.group_topk(m, groups, 10, mode="most_pleasure", member_ratings=True)
    assert users.tolist() == [3, 50, 7] and offsets.tolist() == [0, 2, 3, 6] and member_row.tolist() == [0, 1, 1, 2, 0, 2]
    from anime_recommendations_amd import weights_io
    P = ops.predict_grid(_cuda(np.asarray(m["U"], np.float32)), _cuda(np.asarray(m["A"], np.float32)),
                         weights_io.model_head(m), users).cpu().numpy()
    _same((gi, gs, gm), G.group_topk(P, offsets, member_row, 10, "max"), 10, "recs.group_topk")
    with pytest.raises(ValueError, match="no embedding row"):
        recs.group_topk(m, [[int(uid.max()) + 1]], 10)


def test_group_recs_component(pipeline):  # noqa: F811
    from anime_recommendations_amd import components as C, ops, weights_io
    work, env = pipeline["work"], pipeline["env"]
    df = pd.read_parquet(pipeline["paths"]["user_stats"])
    ids = [int(u) for u in df.user_id.unique()[[5, 40, 77]]]
    m = _model()
    anime_df = C.load_anime_df(pipeline["paths"]["all_anime"])
    syn_df = C.load_synopses(pipeline["paths"]["synopses"])
    user_ids, anime_ids = C.index_tables(m, df)
    # no --group_users: the selected user alone, model_recs' list
    _run("group_recs", _flags(ids[0]), str(work), env)
    got = pd.read_csv(work / ("Group_%d_model_recs.csv" % ids[0]))
    plain = C.model_recs_frame(m["U"], m["A"], weights_io.model_head(m), user_ids, anime_ids, df, anime_df, syn_df, ids[0],
                               10, types=["TV", "Movie"])
    assert got.columns.tolist() == plain.columns.tolist() + ["Min_prediction", "Max_prediction", "User_%d" % ids[0]]
    assert got["Name"].tolist() == plain["Name"].tolist() and len(got) == 10
    assert np.array_equal(got["Prediction"].to_numpy().astype(np.float32), plain["Prediction"].to_numpy())
    # three users under least_misery
    _run("group_recs", _flags(ids[0], group_users=str(ids), group_strategy="least_misery"), str(work), env)
    got = pd.read_csv(work / ("Group_%d_%d_%d_model_recs.csv" % tuple(ids)))
    assert len(got) == 10 and got["Type"].isin(["TV", "Movie"]).all()
    assert np.array_equal(got["Prediction"].to_numpy(), got["Min_prediction"].to_numpy())
    rows = [int(np.nonzero(np.asarray(user_ids) == u)[0][0]) for u in ids]
    P = ops.predict_grid(_cuda(np.asarray(m["U"], np.float32)), _cuda(np.asarray(m["A"], np.float32)),
                         weights_io.model_head(m), rows).cpu().numpy()
    listed = pd.Index(np.asarray(anime_ids)).get_indexer(got["anime_id"])
    assert (listed >= 0).all()
    for i, u in enumerate(ids):
        assert np.array_equal(got["User_%d" % u].to_numpy().astype(np.float32), P[i, listed]), u
    cols = np.stack([got["User_%d" % u].to_numpy() for u in ids])
    assert np.array_equal(got["Min_prediction"].to_numpy(), cols.min(axis=0))
    assert np.array_equal(got["Max_prediction"].to_numpy(), cols.max(axis=0))
    assert (np.diff(got["Prediction"].to_numpy()) <= 0).all()
    assert not (set(got["anime_id"]) & set(df[df.user_id.isin(ids)].anime_id))
