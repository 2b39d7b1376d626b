"""CPU tests of group recommendations: the NumPy restatement checks itself, recs.group_csr, the size query and the
argument checks of anirec_group_topk (none needs a device), the binding, and the group_recs component's flag surface."""
import ctypes
import os

import numpy as np
import pytest

import group_restatement as G
from component_cli import load_component
from rank_restatement import score_key

from anime_recommendations_amd import _lib, build, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _grid(seed=0, n_u=6, n_a=70):
    return np.random.default_rng(seed).normal(size=(n_u, n_a)).astype(np.float32)


# ---- the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.MODES)
def test_one_member_group_is_a_masked_argsort_of_its_row(mode):
    P = _grid()
    P[2, 5] = P[2, 9] = P[2, 30]                                # ties: ascending index
    P[2, 11] = np.nan                                           # NaN: after every number
    watched = np.random.default_rng(1).random(P.shape) < 0.3
    watched[2, [5, 9, 11, 30]] = False
    idx, score, mp = G.group_topk(P, [0, 1], [2], 80, mode, watched=watched)
    cand = np.nonzero(~watched[2])[0]
    finite = cand[~np.isnan(P[2, cand])]
    want = finite[np.argsort(-P[2, finite].astype(np.float64), kind="stable")].tolist() + [11]
    assert idx[0, :len(want)].tolist() == want and (idx[0, len(want):] == -1).all()
    assert np.array_equal(_bits(score[0, :len(want)]), _bits(P[2, want])) and np.isnan(score[0, len(want):]).all()
    assert np.array_equal(_bits(mp[0]), _bits(score[0]))
    assert want.index(5) + 1 == want.index(9) and want.index(9) + 1 == want.index(30)


@pytest.mark.parametrize("copies", [2, 4])
def test_mean_of_copies_of_one_member_is_the_row(copies):
    """p + p and 2p + 2p are exact doublings, and the quotient by 2 or 4 is exact: the row's bits (subnormals aside)"""
    P = _grid(3)
    P[1, 0], P[1, 1], P[1, 2] = np.float32(3.0e38), np.float32(-0.0), np.nan     # 2p overflows: the mean is inf, not p
    agg = G.aggregate(P[[1] * copies], "mean")
    assert np.array_equal(_bits(agg[1:]), _bits(P[1, 1:])) and np.isinf(agg[0])
    one = G.group_topk(P[:, 3:], [0, 1], [1], 70, "mean")
    many = G.group_topk(P[:, 3:], [0, copies], [1] * copies, 70, "mean")
    assert np.array_equal(one[0], many[0]) and np.array_equal(_bits(one[1]), _bits(many[1]))


def test_min_max_nan_and_signed_zero_rules():
    f = np.float32
    nan, pz, nz = f(np.nan), f(0.0), f(-0.0)
    Pm = np.array([[1, nan, 1, pz, nz, 2, nan],
                   [nan, 1, 3, nz, pz, 1, 0.5],
                   [0.5, 0.5, 2, pz, nz, 3, 0.25]], np.float32)
    lo, hi = G.aggregate(Pm, "min"), G.aggregate(Pm, "max")
    # a NaN met at i >= 1 replaces the value and a later number cannot replace a NaN; a NaN at p_0 stays
    assert np.isnan(lo[[0, 1, 6]]).all() and np.isnan(hi[[0, 1, 6]]).all()
    assert lo[2] == 1 and hi[2] == 3 and lo[5] == 1 and hi[5] == 3
    # +0 and -0 compare equal: the earlier member stays, in both modes
    assert _bits(lo[3:5]).tolist() == _bits(np.array([pz, nz])).tolist() == _bits(hi[3:5]).tolist()
    mean = G.aggregate(Pm, "mean")
    assert np.isnan(mean[[0, 1, 6]]).all() and mean[2] == f(2.0) and mean[5] == f(2.0)


def test_floor_rule_with_a_nan_rating():
    f = np.float32
    P = np.array([[0.9, 0.2, np.nan, 0.5, 0.5],
                  [0.8, 0.9, 0.7, 0.5, 0.4999]], np.float32)
    idx, score, _ = G.group_topk(P, [0, 2], [0, 1], 5, "min", floor=f(0.5))
    # anime 1 (0.2 < floor) and 4 (0.4999 < floor) go; anime 2 stays (NaN < floor is false) and ranks last; 3 (== floor) stays
    assert idx[0].tolist() == [0, 3, 2, -1, -1] and np.isnan(score[0, 2:]).all()
    assert G.group_topk(P, [0, 2], [0, 1], 5, "min", floor=f(-np.inf))[0][0].tolist() == [0, 3, 4, 1, 2]
    assert score_key(np.array([np.nan], np.float32))[0] == 1


def test_padding_empty_groups_and_member_rows():
    P = _grid(5)
    watched = np.zeros(P.shape, bool)
    watched[4] = True                                           # a member who has watched everything
    exclude = np.zeros((3, P.shape[1]), bool)
    exclude[0, :60] = True
    idx, score, mp = G.group_topk(P, [0, 2, 2, 4], [0, 1, 4, 3], 12, "mean", watched=watched, exclude=exclude)
    assert (idx[0, :10] >= 60).all() and (idx[0, 10:] == -1).all() and np.isnan(score[0, 10:]).all()
    assert (idx[1:] == -1).all() and np.isnan(score[1:]).all() and np.isnan(mp[2:]).all()
    assert np.array_equal(_bits(mp[1, :10]), _bits(P[1, idx[0, :10]])) and np.isnan(mp[:2, 10:]).all()


# ---- recs.group_csr ---------------------------------------------------------------------------------------------
def test_group_csr():
    ids = np.array([70, 10, 50, 30, 90])
    users, offsets, member_row = recs.group_csr([[30, 10], [10, 10, 90], [], [30]], ids)
    assert users.tolist() == [3, 1, 4]                          # each distinct user once, in order of first appearance
    assert offsets.tolist() == [0, 2, 5, 5, 6]
    assert member_row.tolist() == [0, 1, 1, 1, 2, 0]            # a user in two groups, a repeated member
    assert member_row.dtype == np.int32
    assert ids[users[member_row]].tolist() == [30, 10, 10, 10, 90, 30]
    with pytest.raises(ValueError, match="11, 12"):
        recs.group_csr([[30, 11], [12]], ids)
    users, offsets, member_row = recs.group_csr([], ids)
    assert len(users) == 0 and offsets.tolist() == [0] and len(member_row) == 0


# ---- the binding, the size query and the entry point's refusals -------------------------------------------------
def test_symbols_bound_and_size_query():
    assert len(_lib.PROTOTYPES["anirec_group_topk"][1]) == 25 and len(_lib.PROTOTYPES["anirec_group_topk_workspace_bytes"][1]) == 5
    assert _lib.PROTOTYPES["anirec_group_topk_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.ABI_VERSION == 5 and "anirec_infer.hip" in build.SOURCES
    assert _lib.GROUP_MAX_MEMBERS == 64 and (_lib.GROUP_MEAN, _lib.GROUP_MIN, _lib.GROUP_MAX) == (0, 1, 2)
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.anirec_abi_version() == 5
    size = lib.anirec_group_topk_workspace_bytes
    good = dict(n_anime=1000, n_users=40, n_groups=12, k=10, dim=128)

    def q(**kw):
        a = dict(good, **kw)
        return size(a["n_anime"], a["n_users"], a["n_groups"], a["k"], a["dim"])

    for kw in (dict(n_anime=0), dict(n_anime=-5), dict(n_users=-1), dict(n_groups=-1), dict(k=0), dict(k=-3), dict(dim=48),
               dict(dim=0), dict(dim=512)):
        assert q(**kw) == 0, kw
    words = (1000 + 31) // 32
    for dim in _lib.WIDTHS:                                     # Ah | Uh, then per group a score row and a mask row
        assert q(dim=dim) >= (1000 + 40) * dim * 4 + 12 * (1000 * 4 + words * 4)
    sizes = [q(k=k) for k in (1, 10, 128, 129, 500, 1000, 5000)]
    assert sizes == sorted(sizes) and sizes[0] == sizes[2] < sizes[3] < sizes[4] < sizes[5] == sizes[6]   # k is capped by n
    assert q(n_groups=1) < q(n_groups=12) < q(n_groups=4096) == q(n_groups=100000)     # batches of at most 4096 groups
    assert q(n_groups=0) == q(n_groups=1) and q(n_users=0) > 0


def test_entry_point_refuses_bad_arguments_without_a_device():
    build.build(verbose=False)
    lib = _lib.load()
    head = _lib.Head(1, 0, 1, 0, 0, 1)

    def call(ptr=None, dim=128, n_anime=100, n_users=10, act=0, n_groups=0, n_members=8, max_members=4, mode=0, floor=0.0,
             k=5, ws_bytes=1 << 30):
        return lib.anirec_group_topk(ptr, ptr, dim, n_anime, ptr, n_users, ctypes.byref(head) if ptr else None, act, None,
                                     ptr, ptr, n_groups, n_members, max_members, None, mode, floor, k, ptr, ptr, None,
                                     ptr, ptr, ws_bytes, None)

    assert call() == 0 and call(floor=float("-inf")) == 0 and call(max_members=64) == 0     # no groups: nothing to do
    fake = 4096         # never followed: every refusal comes before anything is enqueued
    for kw in (dict(dim=48), dict(dim=0), dict(n_anime=0), dict(n_users=-1), dict(act=5), dict(act=-1), dict(n_groups=-1),
               dict(n_members=-1), dict(max_members=0), dict(max_members=65), dict(mode=3), dict(mode=-1),
               dict(floor=float("nan")), dict(k=0), dict(k=-1)):
        assert call(**kw) == -1, kw
        assert call(**dict(dict(n_groups=3, ptr=fake), **kw)) == -1, kw
    assert call(n_groups=3) == -1                               # NULL buffers with work to do
    assert call(n_groups=3, ptr=fake, ws_bytes=1000) == -3      # and a workspace below one group's share


def test_ops_refusals_need_no_gpu():
    import torch
    U, A = torch.zeros(10, 128), torch.zeros(200, 128)
    head = dict(w=1, b=0, gamma=1, beta=0, mov_mean=0, mov_var=1)
    for mode, want in (("mean", 0), ("MEAN", 0), ("least_misery", 1), ("Min", 1), ("most_pleasure", 2), ("MAX", 2),
                       (" Least_Misery ", 1)):
        assert ops.group_mode(mode) == want
    with pytest.raises(ValueError, match="least_misery"):
        ops.group_topk(U, A, head, [0, 1], [0, 2], [0, 1], 5, mode="median")
    with pytest.raises(ValueError, match="k must be >= 1"):
        ops.group_topk(U, A, head, [0, 1], [0, 2], [0, 1], 0)
    with pytest.raises(ValueError, match="NaN"):
        ops.group_topk(U, A, head, [0, 1], [0, 2], [0, 1], 5, floor=float("nan"))
    with pytest.raises(ValueError, match="65 members is above the limit of 64"):
        ops.group_topk(U, A, head, [0, 1], [0, 65], [0] * 65, 5)


# ---- the component's flag surface -------------------------------------------------------------------------------
def test_group_recs_parser_and_mlproject_agree():
    from anime_recommendations_amd import components as C
    mod, ref = load_component("group_recs"), load_component("model_recs")
    assert mod.STR_FLAGS == ref.STR_FLAGS and mod.BOOL_FLAGS == ref.BOOL_FLAGS       # the model_recs flag set as it is
    assert mod.OPTIONAL_FLAGS == {"group_users": "[]", "group_strategy": "mean", "group_floor": None}
    assert C.GROUP_STRATEGIES == ("mean", "least_misery", "most_pleasure")
    assert all(s in _lib.GROUP_MODES for s in C.GROUP_STRATEGIES)
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert ns.group_users == [] and ns.group_strategy == "mean" and ns.group_floor is None
    assert sorted(vars(ns)) == sorted(ref.STR_FLAGS + ref.BOOL_FLAGS + ["group_users", "group_strategy", "group_floor"])
    ns = parser.parse_args(argv + ["--group_users", "[5, 9, 5]", "--group_strategy", "Least_Misery", "--group_floor", "0.4"])
    assert ns.group_users == [5, 9, 5] and ns.group_strategy == "least_misery" and ns.group_floor == 0.4
    ns = parser.parse_args(argv + ["--group_users", "", "--group_floor", "none"])
    assert ns.group_users == [] and ns.group_floor is None
    for bad in (["--group_strategy", "median"], ["--group_floor", "nan"], ["--group_floor", "low"], ["--group_users", "[a"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    assert C.group_label([7]) == "7" and C.group_label(range(1, 9)) == "1_2_3_4_5_6_7_8"
    assert C.group_label(range(3, 12)) == "3_and_8_more"
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "group_recs", "MLproject")))
    assert ml["name"] == "group_recs" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    want = list(yaml.safe_load(open(os.path.join(ROOT, "model_recs", "MLproject")))["entry_points"]["main"]["parameters"])
    assert list(params) == want + ["group_users", "group_strategy", "group_floor"]
    assert all(v["description"] for v in params.values()) and all(v["type"] == "str" for v in params.values())
    assert {k: v["default"] for k, v in params.items() if "default" in v} == \
        {"group_users": "[]", "group_strategy": "mean", "group_floor": "none"}
    assert main["command"] == "python group_recs.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert yaml.safe_load(open(os.path.join(ROOT, "group_recs", "conda.yml")))["name"] == "group_recs"
