"""CPU tests of the split fold-in (anirec_fold_in_split) and of the new_anime component's host half: the float32
restatement's distance from the float64 one on the GPU tests' inputs (the figure their tolerance is built on), the
chunk-map builder, the host half of recs.fold_in_anime, recs.append_anime, the new symbols in the header and the
binding, the entry point's checks that need no device, and the component's flag surface."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

import foldin_cases as K
import foldin_split_cases as S
from component_cli import load_component
from anime_recommendations_amd import _lib, build, ops, recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("anirec_fold_in_split_workspace_bytes", "anirec_fold_in_split")


@pytest.mark.parametrize("dim,loss,act", S.CASES)
def test_float32_restatement_stays_within_the_recorded_distance(dim, loss, act):
    """foldin_cases.ROW_DEV and LOSS_DEV bound the float32 restatement on the very inputs of the GPU tests, every row
    and step count.  (Both restatements assert the kink margin on every step.)"""
    r64, r32 = S.reference(dim, loss, act), S.reference(dim, loss, act, "float32")
    has = np.array(S.LENGTHS) > 0
    for s in S.STEPS:
        d_row = np.abs(r32[s][0].astype(np.float64) - r64[s][0]).max()
        d_loss = np.abs(r32[s][1][has].astype(np.float64) - r64[s][1][has]).max()
        print("float32 restatement dim %d %s %s steps %d: row %.3g loss %.3g" % (dim, loss, act, s, d_row, d_loss))
        assert d_row <= K.ROW_DEV and d_loss <= K.LOSS_DEV
        assert np.isnan(r64[s][1][~has]).all() and np.isnan(r32[s][1][~has]).all()
    # it is a fit: the loss at the final row is below the loss at the start row for every row with ratings
    assert (r64[max(S.STEPS)][1][has] < r64[0][1][has]).all()
    assert np.array_equal(r64[0][0], S.case_inputs(dim, loss, act)[5].astype(np.float64))


def test_case_lists_are_the_ones_described():
    T, head, off, idx, t, init = S.case_inputs(128, "binary_crossentropy", "sigmoid")
    assert T.shape == (S.N_TABLE, 128) and not T[S.ZERO_ROW].any() and np.diff(off).tolist() == list(S.LENGTHS)
    assert t[off[1]] == np.float32(0.9) and set(np.round(t * 10).astype(int)) <= set(range(11))
    j = S.LENGTHS.index(1025)
    assert idx[off[j] + 1024] == S.ZERO_ROW and idx.min() >= 0 and idx.max() < S.N_TABLE
    assert len(np.unique(idx[off[-2]:off[-1]])) < 5000                   # drawn with replacement
    tb = S.case_inputs(32, "mean_absolute_error", "relu")[4]
    assert set(tb.tolist()) <= {0.0, 1.0}
    assert ops.FOLD_CHUNK == S.CHUNK == 1024
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    assert re.search(r"#define ANIREC_FOLD_CHUNK 1024\b", src)


def test_chunk_map_builder():
    C = ops.FOLD_CHUNK
    lens = [0, 1, C - 1, C, C + 1, 0, 2 * C, 2 * C + 1, 0, 5000, 0]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c_off, c_row = ops.fold_chunk_map(off)
    assert c_off.dtype == np.int32 and c_row.dtype == np.int32
    counts = [0, 1, 1, 1, 2, 0, 2, 3, 0, 5, 0]
    assert c_off.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert c_row.tolist() == [1, 2, 3, 4, 4, 6, 6, 7, 7, 7, 9, 9, 9, 9, 9] and len(c_row) == c_off[-1]
    # no rows, and nothing but empty lists
    c_off, c_row = ops.fold_chunk_map([0])
    assert c_off.tolist() == [0] and len(c_row) == 0
    c_off, c_row = ops.fold_chunk_map([0, 0, 0])
    assert c_off.tolist() == [0, 0, 0] and len(c_row) == 0
    # a decreasing pair counts no chunks (the kernel poisons that row); the next row spans both lists
    c_off, c_row = ops.fold_chunk_map([0, 3000, 2990, 3100])
    assert c_off.tolist() == [0, 3, 3, 4] and c_row.tolist() == [0, 0, 0, 2]


def _model(n_users=6, n_anime=9, dim=32):
    rng = np.random.default_rng(3)
    return dict(U=rng.standard_normal((n_users, dim)).astype(np.float32) * 0.05,
                A=rng.standard_normal((n_anime, dim)).astype(np.float32) * 0.05,
                head=dict(w=1.0, b=0.0, gamma=1.0, beta=0.0, mov_mean=0.0, mov_var=1.0), activation="sigmoid", loss=None,
                user_ids=np.arange(n_users) * 10 + 100, anime_ids=np.array([50, 7, 19, 3, 88, 41, 12, 66, 5]))


def test_fold_in_anime_csr_groups_drops_and_refuses():
    m = _model()                                                             # users 100, 110, .. 150
    frame = pd.DataFrame({"anime_id": [901, 77, 901, 77, 6, 901, 77],
                          "user_id": [120, 100, 1000, 150, 2000, 120, 110],
                          "rating": [0.5, 1.0, 0.3, 0.0, 0.7, 0.9, 0.2]})
    ids, off, u_idx, rat, dropped = recs.fold_in_anime_csr(frame, m["user_ids"], m["anime_ids"])
    assert ids.tolist() == [901, 77, 6] and ids.dtype == np.int64            # order of first appearance
    assert off.tolist() == [0, 2, 5, 5] and off.dtype == np.int64            # anime 6 keeps a row and no ratings
    assert u_idx.tolist() == [2, 2, 0, 5, 1] and u_idx.dtype == np.int32     # frame order per anime, the repeat kept
    assert rat.tolist() == [np.float32(x) for x in (0.5, 0.9, 1.0, 0.0, 0.2)] and rat.dtype == np.float32
    assert dropped == 2
    ids, off, u_idx, rat, dropped = recs.fold_in_anime_csr(frame.iloc[:0], m["user_ids"], m["anime_ids"])
    assert len(ids) == 0 and off.tolist() == [0] and len(u_idx) == 0 and dropped == 0
    # anime the model holds already are refused by name
    bad = pd.concat([frame, pd.DataFrame({"anime_id": [19, 88, 19], "user_id": [100, 100, 110], "rating": [0.1] * 3})])
    with pytest.raises(ValueError, match=r"fold_in_anime: anime id\(s\) 19, 88 already"):
        recs.fold_in_anime_csr(bad, m["user_ids"], m["anime_ids"])
    with pytest.raises(ValueError, match="id tables"):
        recs.fold_in_anime(dict(m, anime_ids=None), frame)
    for wrong in (float("nan"), 7.0, -0.1):
        broken = frame.copy()
        broken.loc[3, "rating"] = wrong
        with pytest.raises(ValueError, match=r"fold_in_anime: ratings must be numbers in \[0, 1\].*1 of 7"):
            recs.fold_in_anime_csr(broken, m["user_ids"], m["anime_ids"])


def test_append_anime_leaves_the_rest_of_the_model_alone():
    m = _model()
    before = {k: np.array(m[k], copy=True) for k in ("U", "A", "user_ids", "anime_ids")}
    rng = np.random.default_rng(5)
    folded = dict(ids=np.array([901, 77], np.int64), rows=rng.standard_normal((2, 32)).astype(np.float32))
    out = recs.append_anime(m, folded)
    assert out["U"] is m["U"] and out["head"] is m["head"] and out["user_ids"] is m["user_ids"]
    assert out["activation"] == "sigmoid" and out["loss"] is None and set(out) == set(m)
    assert out["A"].dtype == np.float32 and out["A"].shape == (11, 32)
    assert out["A"][:9].tobytes() == before["A"].tobytes() and out["A"][9:].tobytes() == folded["rows"].tobytes()
    assert out["anime_ids"].tolist() == before["anime_ids"].tolist() + [901, 77]
    assert out["anime_ids"].dtype == before["anime_ids"].dtype
    for k, v in before.items():                                              # the input model is not modified
        assert np.asarray(m[k]).tobytes() == v.tobytes()
    import torch
    same = recs.append_anime(m, dict(folded, rows=torch.from_numpy(folded["rows"])))      # rows as a tensor
    assert same["A"].tobytes() == out["A"].tobytes()


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "anirec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(anirec_[a-z0-9_]+)\s*\(", src))


def test_new_symbols_declared_bound_and_exported():
    names = _declared_functions()
    for n in NEW_SYMBOLS:
        assert n in names, "include/anirec.h does not declare %s" % n
        assert n in _lib.PROTOTYPES, "no ctypes prototype for %s" % n
    assert len(_lib.PROTOTYPES["anirec_fold_in_split"][1]) == 23
    assert len(_lib.PROTOTYPES["anirec_fold_in_split_workspace_bytes"][1]) == 4
    assert _lib.ABI_VERSION == 5
    build.build(verbose=False)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS) and lib.anirec_abi_version() == 5


def test_split_entry_point_checks_need_no_gpu():
    """the size query, the argument checks and the empty call return before anything touches a device"""
    build.build(verbose=False)
    lib = _lib.load()
    size = lib.anirec_fold_in_split_workspace_bytes
    for dim in _lib.WIDTHS:
        # the normalised table, m, v, one partial row and loss per chunk, the row flags and the map flag
        assert size(211, 9, 16, dim) == (211 + 9 + 9 + 16) * dim * 4 + 16 * 4 + 48
        assert size(211, 0, 0, dim) == 211 * dim * 4 + 16
        assert size(211, 9, 16, dim) % 16 == 0
    for dim in (0, 16, 48, 100, 512):
        assert size(211, 9, 16, dim) == 0
    assert size(0, 9, 16, 128) == 0 and size(211, -1, 16, 128) == 0 and size(211, 9, -1, 128) == 0
    h = _lib.Head(1, 0, 1, 0, 0, 1)

    def call(dim=128, n_table=211, act=0, loss=0, n_new=0, n_chunks=0, steps=10, ptr=None, ws_bytes=0):
        return lib.anirec_fold_in_split(ptr, dim, n_table, ctypes.byref(h), act, loss, 1e-4, ptr, ptr, ptr, n_new, ptr, ptr,
                                        n_chunks, ptr, ptr, steps, ptr, ptr, ptr, ptr, ws_bytes, None)

    for dim in (0, 16, 48, 100, 512):
        assert call(dim=dim) == -1                              # ANIREC_EINVAL, whatever else the call holds
    assert call(act=5) == -1 and call(act=-1) == -1 and call(loss=5) == -1 and call(loss=-1) == -1
    assert call(steps=-1) == -1 and call(n_new=-1) == -1 and call(n_table=0) == -1 and call(n_chunks=-1) == -1
    for dim in _lib.WIDTHS:
        assert call(dim=dim) == 0 and call(dim=dim, steps=0) == 0       # no rows: nothing to do
    assert call(n_new=3, n_chunks=3) == -1                      # NULL buffers with work to do
    # a workspace one byte short is refused before anything is enqueued (the pointers are never followed)
    assert call(n_new=3, n_chunks=3, ptr=4096, ws_bytes=size(211, 3, 3, 128) - 1) == -1


def test_new_anime_parser_and_mlproject_agree():
    mod, ref = load_component("new_anime"), load_component("similar_anime")
    extra = ["new_ratings", "fold_steps", "fold_lr", "audience_number"]
    # the similar_anime flags plus the fold-in ones; --anime_query stays a flag, now an optional id of the file
    assert sorted(mod.STR_FLAGS + mod.BOOL_FLAGS + ["anime_query"]) == sorted(ref.STR_FLAGS + ref.BOOL_FLAGS + extra)
    assert mod.OPTIONAL_FLAGS == ["anime_query", "output_model"]
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert ns.anime_query == "None" and ns.output_model == "None" and ns.new_ratings == "x" and ns.save_sim_anime is True
    assert parser.parse_args(argv + ["--anime_query", "77", "--output_model", "m.h5"]).output_model == "m.h5"
    with pytest.raises(SystemExit):
        parser.parse_args(argv[2:])
    frame = pd.DataFrame({"user_id": [1, 2], "anime_id": [901, 77], "rating": [0.5, 0.5]})
    assert mod.select_anime(ns, frame) == 901                     # the first anime of the file
    ns.anime_query = "77"
    assert mod.select_anime(ns, frame) == 77
    ns.anime_query = "Cowboy Bebop"                               # a new anime has no title row to look up
    with pytest.raises(ValueError, match="anime id of the new ratings file"):
        mod.select_anime(ns, frame)
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "new_anime", "MLproject")))
    assert ml["name"] == "new_anime" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + mod.BOOL_FLAGS + mod.OPTIONAL_FLAGS
    assert all(v["type"] == "str" and v["description"] for v in params.values())
    assert [k for k, v in params.items() if "default" in v] == mod.OPTIONAL_FLAGS
    assert all(params[k]["default"] in (None, "None") for k in mod.OPTIONAL_FLAGS)
    assert main["command"] == "python new_anime.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert os.path.exists(os.path.join(ROOT, "new_anime", "conda.yml"))
