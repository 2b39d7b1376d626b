"""CPU tests of the fold-in of new users: the restatement's closed-form gradient against torch.autograd in fp64, the
float32 restatement's distance from the float64 one on the GPU tests' inputs (the figure their tolerance is built on),
the host half of recs.fold_in_users, the new symbols in the header and the binding, the entry point's checks that
need no device, and the new_user_recs component's flag surface."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import foldin_cases as K
import foldin_restatement as F
from component_cli import load_component
from anime_recommendations_amd import _lib, build, components as C, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("anirec_fold_in_workspace_bytes", "anirec_fold_in")
_T_ACT = {"sigmoid": torch.sigmoid, "linear": lambda y: y, "tanh": torch.tanh, "relu": torch.relu,
          "softplus": torch.nn.functional.softplus}


def _torch_loss(u, Ah, t, hs, hb, l2, loss, act):
    """the model's loss of one user row in torch: l2_normalize, the dot with the normalised anime rows, the folded
    head, Keras' losses as published"""
    uh = u * torch.rsqrt(torch.clamp((u * u).sum(), min=F.L2N_EPS))
    y = (Ah * uh).sum(1) * hs + hb
    if loss == "binary_crossentropy" and act == "sigmoid":
        data = torch.nn.functional.binary_cross_entropy_with_logits(y, t)
    else:
        p = _T_ACT[act](y)
        e = p - t
        if loss == "binary_crossentropy":
            eps = float(np.float32(1e-7))             # Keras' epsilon and 1 - epsilon as the float32 values they are
            q = torch.clamp(p, eps, float(np.float32(1) - np.float32(1e-7)))
            data = -(t * torch.log(q + eps) + (1 - t) * torch.log(1 - q + eps)).mean()
        elif loss == "mean_squared_error":
            data = (e * e).mean()
        elif loss == "mean_absolute_error":
            data = e.abs().mean()
        elif loss == "huber":
            data = torch.where(e.abs() <= 1, 0.5 * e * e, e.abs() - 0.5).mean()
        else:
            data = (e + torch.nn.functional.softplus(-2 * e) - np.log(2.0)).mean()
    return data + l2 * (u * u).sum()


@pytest.mark.parametrize("loss,act", K.HEAD_PAIRS)
def test_closed_form_gradient_matches_autograd_fp64(loss, act):
    """the tolerances of tests/test_oracle.py's autograd cross-check: 1e-12 on the loss, 1e-14 on the gradient"""
    A, head, off, idx, t, init = K.case_inputs(128, loss, act)
    hs, hb = (float(x) for x in F.head_affine_f32(head))
    Ah64 = F.normalised_rows(A, np.float64)
    tol_l, tol_g = 1e-12, 1e-14
    for j in (1, 4, 8, 15):                                   # 1, 5, 16 and 700 ratings
        sl = slice(off[j], off[j + 1])
        rows, tt = Ah64[idx[sl]], t[sl].astype(np.float64)
        u = init[j].astype(np.float64)
        L, g, _ = F.loss_and_grad(u, rows, tt, hs, hb, K.L2, loss, act, np.float64)
        tu = torch.tensor(u, requires_grad=True)
        total = _torch_loss(tu, torch.tensor(rows), torch.tensor(tt), hs, hb, K.L2, loss, act)
        total.backward()
        assert abs(float(total.detach()) - float(L)) < tol_l
        np.testing.assert_allclose(g, tu.grad.numpy(), rtol=0, atol=tol_g)


@pytest.mark.parametrize("dim,loss,act", K.CASES + K.FAR_CASES)
def test_float32_restatement_stays_within_the_recorded_distance(dim, loss, act):
    """ROW_DEV and LOSS_DEV are what the GPU tolerance is 8 x of: they must bound the float32 restatement on the very
    inputs of the GPU tests.  (Both restatements assert the kink margin on every step.)"""
    r64, r32 = K.reference(dim, loss, act), K.reference(dim, loss, act, "float32")
    ROW_DEV, LOSS_DEV = K.deviations(dim, loss, act)
    for s in K.STEPS:
        assert np.abs(r32[s][0].astype(np.float64) - r64[s][0]).max() <= ROW_DEV
        has = np.array(K.LENGTHS) > 0
        assert np.isnan(r64[s][1][~has]).all() and np.isnan(r32[s][1][~has]).all()
        assert np.abs(r32[s][1][has].astype(np.float64) - r64[s][1][has]).max() <= LOSS_DEV
    # it is a fit: the loss at the final row is below the loss at the start row for every user with ratings
    assert (r64[100][1][has] < r64[0][1][has]).all()
    assert np.array_equal(r64[0][0], K.case_inputs(dim, loss, act)[5].astype(np.float64))


def test_restatement_steps_and_empty_list():
    A, head, off, idx, t, init = K.case_inputs(32, "binary_crossentropy", "sigmoid")
    r = F.fold_in(A, head, idx[:0], t[:0], init[0], K.alphas(8))
    assert np.array_equal(r["row"], init[0].astype(np.float64)) and np.isnan(r["loss"]) and r["losses"] == []
    sl = slice(off[5], off[6])
    r8 = F.fold_in(A, head, idx[sl], t[sl], init[5], K.alphas(8), snapshots=(0, 3, 8))
    r3 = F.fold_in(A, head, idx[sl], t[sl], init[5], K.alphas(3))
    assert len(r8["losses"]) == 8 and r8["losses"][0] == r8["snap"][0][1]        # L_1 is the loss at the start row
    assert np.array_equal(r8["snap"][3][0], r3["row"]) and r8["snap"][3][1] == r3["loss"]
    assert np.array_equal(r8["snap"][8][0], r8["row"]) and r8["snap"][8][1] == r8["loss"]
    # a repeated rating counts twice: the list [a, a] is not the list [a]
    one = F.fold_in(A, head, [3], [0.9], init[1], K.alphas(2))
    two = F.fold_in(A, head, [3, 3, 40], [0.9, 0.9, 0.1], init[1], K.alphas(2))
    ref = F.fold_in(A, head, [3, 40], [0.9, 0.1], init[1], K.alphas(2))
    assert not np.array_equal(two["row"], ref["row"]) and not np.array_equal(one["row"], ref["row"])
    # the kink assertion fires when a rating sits on a jump
    hs, hb = F.head_affine_f32(head)
    uh = init[1].astype(np.float64) / np.linalg.norm(init[1].astype(np.float64))
    p0 = float(F.normalised_rows(A, np.float64)[3] @ uh) * float(hs) + float(hb)    # the linear head's p at the start row
    with pytest.raises(AssertionError, match="gradient jump"):
        F.fold_in(A, head, [3], [F.f32(p0)], init[1], K.alphas(2), loss="mean_absolute_error", act="linear")


def _model(n_users=6, n_anime=9, dim=32):
    rng = np.random.default_rng(3)
    return dict(U=rng.standard_normal((n_users, dim)).astype(np.float32) * 0.05,
                A=rng.standard_normal((n_anime, dim)).astype(np.float32) * 0.05,
                head=dict(w=1.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0), activation="sigmoid", loss=None,
                user_ids=np.arange(n_users) * 10 + 100, anime_ids=np.array([50, 7, 19, 3, 88, 41, 12, 66, 5]))


def test_fold_in_csr_groups_drops_and_refuses():
    m = _model()
    frame = pd.DataFrame({"user_id": [901, 77, 901, 77, 5, 901, 77],
                          "anime_id": [19, 50, 1000, 5, 2000, 19, 7],
                          "rating": [0.5, 1.0, 0.3, 0.0, 0.7, 0.9, 0.2]})
    ids, off, a_idx, rat, dropped = recs.fold_in_csr(frame, m["user_ids"], m["anime_ids"])
    assert ids.tolist() == [901, 77, 5] and ids.dtype == np.int64            # order of first appearance
    assert off.tolist() == [0, 2, 5, 5] and off.dtype == np.int64            # user 5 keeps a row and no ratings
    assert a_idx.tolist() == [2, 2, 0, 8, 1] and a_idx.dtype == np.int32     # frame order per user, the repeat kept
    assert rat.tolist() == [np.float32(x) for x in (0.5, 0.9, 1.0, 0.0, 0.2)] and rat.dtype == np.float32
    assert dropped == 2
    # an empty frame is an empty CSR
    ids, off, a_idx, rat, dropped = recs.fold_in_csr(frame.iloc[:0], m["user_ids"], m["anime_ids"])
    assert len(ids) == 0 and off.tolist() == [0] and len(a_idx) == 0 and dropped == 0
    # users the model holds already are refused by name
    bad = pd.concat([frame, pd.DataFrame({"user_id": [120, 150, 120], "anime_id": [7, 7, 3], "rating": [0.1] * 3})])
    with pytest.raises(ValueError, match=r"120, 150"):
        recs.fold_in_csr(bad, m["user_ids"], m["anime_ids"])
    with pytest.raises(ValueError, match="id tables"):
        recs.fold_in_users(dict(m, user_ids=None), frame)
    # ratings are the scaled ones: NaN or a raw 0..10 score is refused before anything reaches the kernel
    for wrong in (float("nan"), 7.0, -0.1):
        broken = frame.copy()
        broken.loc[3, "rating"] = wrong
        with pytest.raises(ValueError, match=r"ratings must be numbers in \[0, 1\].*1 of 7"):
            recs.fold_in_csr(broken, m["user_ids"], m["anime_ids"])


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", src))


def test_new_symbols_declared_bound_and_exported():
    names = _declared_functions()
    for n in NEW_SYMBOLS:
        assert n in names, "include/anirec.h does not declare %s" % n
        assert n in _lib.PROTOTYPES, "no ctypes prototype for %s" % n
    assert set(_lib.PROTOTYPES) == names                       # test_abi's rule: the binding lists the header, no more
    assert len(_lib.PROTOTYPES["anirec_fold_in"][1]) == 20 and len(_lib.PROTOTYPES["anirec_fold_in_workspace_bytes"][1]) == 3
    assert _lib.ABI_VERSION == 5
    assert "anirec_foldin.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS) and lib.anirec_abi_version() == 5


def test_fold_in_entry_point_checks_need_no_gpu():
    """the size query, the argument checks and the empty call return before anything touches a device"""
    build.build(verbose=False)
    lib = _lib.load()
    for dim in _lib.WIDTHS:
        assert lib.anirec_fold_in_workspace_bytes(97, 5, dim) == 97 * dim * 4
        assert lib.anirec_fold_in_workspace_bytes(97, 0, dim) == 97 * dim * 4
    for dim in (0, 16, 48, 100, 512):
        assert lib.anirec_fold_in_workspace_bytes(97, 5, dim) == 0
    assert lib.anirec_fold_in_workspace_bytes(0, 5, 128) == 0 and lib.anirec_fold_in_workspace_bytes(97, -1, 128) == 0
    h = _lib.Head(1, 0, 1, 0, 0, 1)

    def call(dim=128, n_anime=97, act=0, loss=0, n_new=0, steps=10, ptr=None, ws_bytes=0):
        return lib.anirec_fold_in(ptr, dim, n_anime, ctypes.byref(h), act, loss, 1e-4, ptr, ptr, ptr, n_new, ptr, ptr,
                                  steps, ptr, ptr, ptr, ptr, ws_bytes, None)

    for dim in (0, 16, 48, 100, 512):
        assert call(dim=dim) == -1                              # ANIREC_EINVAL, whatever else the call holds
    assert call(act=5) == -1 and call(act=-1) == -1 and call(loss=5) == -1 and call(loss=-1) == -1
    assert call(steps=-1) == -1 and call(n_new=-1) == -1 and call(n_anime=0) == -1
    for dim in _lib.WIDTHS:
        assert call(dim=dim) == 0 and call(dim=dim, steps=0) == 0       # no new users: nothing to do
    assert call(n_new=3) == -1                                  # NULL buffers with work to do
    # a workspace one byte short is refused before anything is enqueued (the pointers are never followed)
    fake = 4096
    assert call(n_new=3, ptr=fake, ws_bytes=97 * 128 * 4 - 1) == -1


def test_new_user_recs_parser_and_mlproject_agree():
    mod, ref = load_component("new_user_recs"), load_component("model_recs")
    extra = ["new_ratings", "fold_steps", "fold_lr", "fold_neighbours"]
    want = ref.STR_FLAGS + ref.BOOL_FLAGS + extra                 # the model_recs flags plus the fold-in ones
    assert sorted(mod.STR_FLAGS + mod.BOOL_FLAGS) == sorted(want) and mod.OPTIONAL_FLAGS == ["user_query"]
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert ns.user_query == "None" and ns.fold_neighbours is True and ns.new_ratings == "x"
    assert parser.parse_args(argv + ["--user_query", "77"]).user_query == "77"
    with pytest.raises(SystemExit):
        parser.parse_args(argv[2:])
    # the queried user: --user_query, else the first of the file — whatever the model_recs flags for a trained user say
    frame = pd.DataFrame({"user_id": [901, 77], "anime_id": [1, 2], "rating": [0.5, 0.5]})
    ns.model_ID_conf, ns.model_user_query = True, "55"
    assert mod.select_user(ns, frame) == 901
    ns.model_ID_conf = False
    assert mod.select_user(ns, frame) == 901
    ns.user_query = "77"
    assert mod.select_user(ns, frame) == 77
    # the MLproject file as mlflow reads it
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "new_user_recs", "MLproject")))
    assert ml["name"] == "new_user_recs" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + mod.BOOL_FLAGS + ["user_query"]
    assert all(v["type"] == "str" and v["description"] for v in params.values())
    assert [k for k, v in params.items() if "default" in v] == ["user_query"] and params["user_query"]["default"] in (None, "None")
    assert main["command"] == "python new_user_recs.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    for comp in ("evaluate", "model_recs"):                       # the same reader takes the components it is modelled on
        assert "main" in yaml.safe_load(open(os.path.join(ROOT, comp, "MLproject")))["entry_points"]
    assert os.path.exists(os.path.join(ROOT, "new_user_recs", "conda.yml"))
