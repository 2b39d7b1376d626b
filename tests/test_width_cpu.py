"""CPU tests of --embedding_size: the width check of trainer.fit (before the engine is touched), the refusals of the
multi-GPU engine and of an engine built for another width, weights files of another width, and the _w twins of the C
ABI (declared, exported, bound, refusing a bad width without a GPU)."""
import json
import os
import subprocess

import numpy as np
import pytest

from anime_recommendations_amd import _lib, data, trainer, weights_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (32, 64, 128, 256)


class _Engine:
    """Stand-in with TrainEngine's interface that records every call it sees (test_metrics_cpu's double, reduced to the
    record): a refusal that comes in time leaves ``calls`` empty."""

    optimizer, loss, activation, metrics = "adam", "binary_crossentropy", "sigmoid", 0

    def __init__(self, width=128):
        import torch
        self.device = torch.device("cpu")
        self.width = width
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **kw):
            self.calls.append(name)
            raise AssertionError("the engine was touched: %s" % name)
        return call


def _table():
    return data.encode_frame(data.synth_user_stats(n_users=40, n_anime=60, n_ratings=1500, seed=3))


@pytest.mark.parametrize("bad", [0, -1, 48, 100, 512])
def test_fit_refuses_other_widths_before_the_engine_is_touched(bad):
    eng = _Engine(width=bad)
    cfg = trainer.FitConfig(epochs=1, batch_size=256, test_size=200, verbose=0, embedding_size=bad)
    with pytest.raises(ValueError) as e:
        trainer.fit(_table(), cfg, engine=eng)
    assert eng.calls == []
    for w in WIDTHS:                                   # the message lists what is supported
        assert str(w) in str(e.value)
    assert repr(bad) in str(e.value)


def test_width_check_takes_the_four_widths_and_nothing_else():
    assert _lib.WIDTHS == WIDTHS and _lib.DIM == 128
    for w in WIDTHS:
        assert _lib.check_width(w) == w and _lib.check_width(np.int64(w)) == w
    for bad in (0, -1, 48, 100, 512, 64.5, "64", None):
        with pytest.raises(ValueError, match="32, 64, 128, 256"):
            _lib.check_width(bad)


@pytest.mark.parametrize("have,want", [(128, 64), (64, 128), (32, 256)])
def test_fit_refuses_an_engine_built_for_another_width(have, want):
    eng = _Engine(width=have)
    cfg = trainer.FitConfig(epochs=1, batch_size=256, test_size=200, verbose=0, embedding_size=want)
    with pytest.raises(ValueError, match="embedding width %d" % have):
        trainer.fit(_table(), cfg, engine=eng)
    assert eng.calls == []


def test_fit_hands_tables_of_the_asked_width_to_the_engine():
    """a supported width passes the checks: the first thing the engine sees are [n, 64] tables"""
    seen = {}

    class Eng(_Engine):
        def set_head(self, **kw):
            seen["head"] = kw

        def set_weights(self, U, A):
            seen["shapes"] = (U.shape, A.shape)
            raise StopIteration

    table = _table()
    cfg = trainer.FitConfig(epochs=1, batch_size=256, test_size=200, verbose=0, embedding_size=64, seed=4)
    with pytest.raises(StopIteration):
        trainer.fit(table, cfg, engine=Eng(width=64))
    assert seen["shapes"] == ((table.n_users, 64), (table.n_anime, 64))
    U, A, w = trainer.init_weights(table.n_users, table.n_anime, 64, 4)
    assert U.shape == (table.n_users, 64) and seen["head"] == {"w": w}


def test_multi_gpu_engine_is_128_only():
    from anime_recommendations_amd.dist import DistTrainEngine
    with pytest.raises(ValueError, match="multi-GPU training is 128-only"):
        DistTrainEngine(100, 50, 16, device="cpu", width=64)
    with pytest.raises(ValueError, match="32, 64, 128, 256"):
        DistTrainEngine(100, 50, 16, device="cpu", width=48)


def test_sharded_inference_never_picks_the_mfma_path_at_another_width(monkeypatch):
    import torch
    from anime_recommendations_amd import dist_infer, ops
    took = []
    monkeypatch.setattr(ops, "cosine_topk_mfma", lambda *a, **kw: took.append("mfma"))
    monkeypatch.setattr(ops, "predict_topk_mfma", lambda *a, **kw: took.append("mfma"))

    def exact(*a, **kw):
        took.append("exact")
        return torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5, 3)
    monkeypatch.setattr(ops, "cosine_topk", exact)
    monkeypatch.setattr(ops, "predict_topk", exact)
    W = torch.zeros(5, 64)
    dist_infer.sharded_cosine_topk(W, 3)
    dist_infer.sharded_predict_topk(W, W, {}, [0, 1, 2, 3, 4], 3)
    assert took == ["exact", "exact"]


def test_mfma_ops_name_the_exact_op_for_another_width(monkeypatch):
    import torch
    from anime_recommendations_amd import ops
    monkeypatch.setattr(ops, "_need_gpu", lambda: None)
    W = torch.zeros(8, 64)
    for fn, args, exact in ((ops.cosine_topk_mfma, (W, [0], 3), "ops.cosine_topk"),
                            (ops.predict_grid_mfma, (W, W, {}, [0]), "ops.predict_grid"),
                            (ops.predict_topk_mfma, (W, W, {}, [0], 3), "ops.predict_topk")):
        with pytest.raises(ValueError) as e:
            fn(*args)
        assert exact in str(e.value) and "128" in str(e.value)


@pytest.mark.parametrize("width", [32, 64, 256])
def test_weights_files_round_trip_other_widths(tmp_path, width):
    rng = np.random.default_rng(width)
    U = rng.normal(0, 0.05, (7, width)).astype(np.float32)
    A = rng.normal(0, 0.05, (5, width)).astype(np.float32)
    head = dict(w=1.1, b=0.2, gamma=0.9, beta=-0.1, mov_mean=0.01, mov_var=0.8)
    opt = {"user_embedding/m": U * 2, "user_embedding/v": U * U, "anime_embedding/m": A * 2,
           "anime_embedding/v": A * A, "head/m": np.zeros(4, np.float32), "head/v": np.ones(4, np.float32),
           "iterations": np.array([12], np.int64)}
    p = str(tmp_path / "m.safetensors")
    weights_io.save_model(p, U, A, head, np.arange(7) * 3, np.arange(5) * 11, optimizer=opt)
    m = weights_io.load_model(p)
    assert m["U"].shape == (7, width) and m["A"].shape == (5, width)
    np.testing.assert_array_equal(m["U"], U)
    np.testing.assert_array_equal(m["A"], A)
    np.testing.assert_array_equal(m["optimizer"]["user_embedding/v"], U * U)
    assert list(m["anime_ids"]) == list(np.arange(5) * 11)
    assert all(abs(m["head"][k] - np.float32(v)) == 0 for k, v in head.items())


# ---- the C ABI -------------------------------------------------------------------------------------------------
TWINS = ("anirec_train_workspace_bytes", "anirec_train_init_reg", "anirec_train_prep", "anirec_train_fwd",
         "anirec_train_head", "anirec_train_bwd", "anirec_train_adam", "anirec_trainer_create", "anirec_eval_metrics",
         "anirec_rownorm", "anirec_cosine_scores", "anirec_cosine_topk", "anirec_cosine_topk_large",
         "anirec_predict_pairs", "anirec_predict_workspace_bytes", "anirec_predict_grid", "anirec_predict_topk",
         "anirec_predict_topk_large_workspace_bytes", "anirec_predict_topk_large")


def test_twins_are_declared_type_checked_and_the_abi_stays_put(tmp_path):
    decl = r'''
#include "anirec.h"
size_t (*a0)(int32_t, int32_t, int32_t) = anirec_train_workspace_bytes_w;
int (*a1)(const anirec_train_desc *, int32_t, void *) = anirec_train_init_reg_w;
int (*a2)(const anirec_train_desc *, int32_t, int32_t, int32_t, void *) = anirec_train_prep_w;
int (*a3)(const anirec_train_desc *, int32_t, void *) = anirec_train_fwd_w;
int (*a4)(const anirec_train_desc *, int32_t, void *) = anirec_train_head_w;
int (*a5)(const anirec_train_desc *, int32_t, void *) = anirec_train_bwd_w;
int (*a6)(const anirec_train_desc *, int32_t, void *) = anirec_train_adam_w;
int (*a7)(const anirec_train_desc *, int32_t, anirec_trainer **) = anirec_trainer_create_w;
int (*a8)(const anirec_train_desc *, int32_t, uint32_t, anirec_metric_acc *, const int32_t *, const int32_t *,
          const float *, int32_t, void *) = anirec_eval_metrics_w;
int (*b0)(const float *, int32_t, int32_t, float *, void *) = anirec_rownorm_w;
int (*b1)(const float *, int32_t, int32_t, int32_t, float *, void *) = anirec_cosine_scores_w;
int (*b2)(const float *, int32_t, int32_t, const int32_t *, int32_t, const uint8_t *, int32_t, int32_t, int32_t *,
          float *, void *, size_t, void *) = anirec_cosine_topk_w;
int (*b3)(const float *, int32_t, int32_t, const int32_t *, int32_t, const uint8_t *, int32_t, int32_t, int32_t *,
          float *, void *, size_t, void *) = anirec_cosine_topk_large_w;
int (*b4)(const float *, const float *, int32_t, const int32_t *, const int32_t *, int32_t, const anirec_head *,
          int32_t, float *, void *) = anirec_predict_pairs_w;
size_t (*b5)(int32_t, int32_t, int32_t, int32_t) = anirec_predict_workspace_bytes_w;
int (*b6)(const float *, const float *, int32_t, int32_t, const int32_t *, int32_t, const anirec_head *, int32_t,
          float *, void *, size_t, void *) = anirec_predict_grid_w;
int (*b7)(const float *, const float *, int32_t, int32_t, const int32_t *, int32_t, const anirec_head *, int32_t,
          const uint32_t *, int32_t, int32_t *, float *, void *, size_t, void *) = anirec_predict_topk_w;
size_t (*b8)(int32_t, int32_t, int32_t, int32_t) = anirec_predict_topk_large_workspace_bytes_w;
int (*b9)(const float *, const float *, int32_t, int32_t, const int32_t *, int32_t, const anirec_head *, int32_t,
          const uint32_t *, int32_t, int32_t *, float *, void *, size_t, void *) = anirec_predict_topk_large_w;
_Static_assert(ANIREC_ABI_VERSION == 5 && ANIREC_DIM == 128 && sizeof(anirec_train_desc) == 176, "ABI");
'''
    d = tmp_path / "decl.c"
    d.write_text(decl)
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(d)])


def test_twins_are_exported_bound_and_refuse_a_bad_width_without_a_gpu():
    from anime_recommendations_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    for n in TWINS:
        assert n + "_w" in _lib.PROTOTYPES and hasattr(lib, n + "_w")
    # the size functions: 0 for a bad width, the old value at 128, a size that follows the width otherwise
    assert lib.anirec_train_workspace_bytes_w(1000, 8, 128) == lib.anirec_train_workspace_bytes(1000, 8)
    assert lib.anirec_predict_workspace_bytes_w(500, 7, 1, 128) == lib.anirec_predict_workspace_bytes(500, 7, 1)
    assert (lib.anirec_predict_topk_large_workspace_bytes_w(500, 7, 300, 128)
            == lib.anirec_predict_topk_large_workspace_bytes(500, 7, 300))
    capC = (1000 + 1000 // _lib.CHUNK + 2 + 3) & ~3
    for w in (32, 64, 256):
        assert (lib.anirec_train_workspace_bytes_w(1000, 8, w) - lib.anirec_train_workspace_bytes(1000, 8)
                == 2 * 2 * capC * 4 * (w - 128))                         # the chunk partial rows P, nothing else
        assert (lib.anirec_predict_workspace_bytes_w(500, 7, 0, w) == (500 + 7) * w * 4)
    for bad in (0, 48, 512, -128):
        assert lib.anirec_train_workspace_bytes_w(1000, 8, bad) == 0
        assert lib.anirec_predict_workspace_bytes_w(500, 7, 1, bad) == 0
        assert lib.anirec_predict_topk_large_workspace_bytes_w(500, 7, 300, bad) == 0
        # (the pointers are never looked at: the width is refused first, and so is a NULL descriptor)
        assert lib.anirec_rownorm_w(None, 4, bad, None, None) == -1
        assert lib.anirec_train_fwd_w(None, bad, None) == -1
        assert lib.anirec_trainer_create_w(None, bad, None) == -1
        assert lib.anirec_eval_metrics_w(None, bad, 0, None, None, None, None, 0, None) == -1


def test_topk_workspace_sizes_keep_their_recorded_values():
    """The four workspace size functions of the exact top-k, value for value against tests/golden/
    topk_workspace_bytes.json (make_topk_workspace_bytes.py, written from the build before the entry points came to
    share one layout description): n, nq and k on both sides of every cap, the 4 GiB halving of a batch, the widths,
    and the invalid arguments that give 0."""
    from anime_recommendations_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    with open(os.path.join(ROOT, "tests", "golden", "topk_workspace_bytes.json")) as f:
        rec = json.load(f)
    assert sorted(rec) == ["anirec_predict_topk_large_workspace_bytes_w", "anirec_predict_workspace_bytes_w",
                           "anirec_topk_large_workspace_bytes", "anirec_topk_workspace_bytes"]
    assert sum(len(v) for v in rec.values()) == 1122
    for name, rows in rec.items():
        fn = getattr(lib, name)
        for args, want in rows:
            assert fn(*args) == want, (name, args)
    # the grid does reach the halving (a 1024-query batch of 350 000-key rows is 1.3 GiB: 4096 users halve, 1024
    # queries do not) and the zeros
    small = dict((tuple(a), v) for a, v in rec["anirec_topk_workspace_bytes"])
    large = dict((tuple(a), v) for a, v in rec["anirec_predict_topk_large_workspace_bytes_w"])
    assert small[(350_000, 4096)] == 4096 * 4 + 2048 * 128 * 8 + 1024 * 350_000 * 4
    assert large[(350_000, 4096, 1, 128)] < 4096 * 350_000 * 4 < 2 * large[(350_000, 4096, 1, 128)]
    assert small[(0, 5)] == 0 and large[(300, 5, 10, 48)] == 0 and large[(300, 5, 0, 128)] == 0


def test_python_mirror_of_the_workspace_follows_the_width():
    from anime_recommendations_amd.engine import workspace_layout
    lib = _lib.load()
    for w in WIDTHS:
        assert workspace_layout(1000, 8, w)["total"] == lib.anirec_train_workspace_bytes_w(1000, 8, w)
    assert workspace_layout(1000, 8) == workspace_layout(1000, 8, 128)
