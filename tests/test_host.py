"""CPU tests of the host side: index contract, artifact store, model container, component
flag surface (against the reference's flag lists), filters, and the epoch driver
(LearningRateScheduler / ModelCheckpoint / EarlyStopping semantics) on a fake engine."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from anime_recommendations_amd import artifacts, components as C, data, trainer, weights_io
from oracle import anirec_oracle as orc
from component_cli import load_component

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_encode_ids_is_first_appearance_order_and_matches_oracle():
    ids = np.array([50, 7, 50, 3, 7, 99, 3])
    idx, uniq = data.encode_ids(ids)
    assert list(uniq) == [50, 7, 3, 99] and list(idx) == [0, 1, 0, 2, 1, 3, 2]
    oi, ou = orc.encode_ids(ids)
    assert (oi == idx).all() and (ou == uniq).all()
    # == the reference's dict construction over Series.unique()
    s = pd.Series(ids)
    m = {x: i for i, x in enumerate(s.unique().tolist())}
    assert (s.map(m).to_numpy() == idx).all()


def test_frame_to_columns_nulls_and_the_id_bounds_it_hands_on():
    """ingest.frame_to_columns (host side of the GPU ingest): NaN in an integer column becomes NULL_I32, the rating
    stays float64 with NaN, and the id bounds (max + 1 of the non-missing ids: the sizes of the direct-index tables)
    are taken while the frame is still on the host, so that preprocess_columns / encode_columns need no pass over the
    device columns for them."""
    import pandas as pd
    import torch
    from anime_recommendations_amd import ingest
    df = pd.DataFrame({"user_id": [3.0, np.nan, 9.0, 0.0], "anime_id": [7, 2, 41, 41], "rating": [1.0, np.nan, 3.5, 0.0],
                       "watching_status": [1.0, 2.0, np.nan, 6.0], "watched_episodes": [0, 1, 1, 12]})
    cols = ingest.frame_to_columns(df, device="cpu")
    assert isinstance(cols, ingest.Columns) and cols.bounds == {"user_id": 10, "anime_id": 42}
    assert cols["user_id"].tolist() == [3, ingest.NULL_I32, 9, 0] and cols["user_id"].dtype == torch.int32
    assert cols["watching_status"].tolist() == [1, 2, ingest.NULL_I32, 6]
    assert cols["rating"].dtype == torch.float64 and bool(torch.isnan(cols["rating"][1])) and float(cols["rating"][2]) == 3.5
    empty = ingest.frame_to_columns(df.iloc[:0], device="cpu")
    assert empty.bounds == {"user_id": 1, "anime_id": 1} and all(v.numel() == 0 for v in empty.values())
    only_null = ingest.frame_to_columns(df.iloc[[1]].assign(anime_id=np.nan), device="cpu")
    assert only_null.bounds == {"user_id": 1, "anime_id": 1}
    with pytest.raises(ValueError):
        ingest.frame_to_columns(df.assign(user_id=[0.5, 1, 2, 3]), device="cpu")        # not an integer column
    with pytest.raises(ValueError):
        ingest.frame_to_columns(df.assign(anime_id=[2 ** 31, 1, 2, 3]), device="cpu")   # does not fit int32
    # a plain dict of columns is still accepted everywhere a Columns is (no bounds: they are computed)
    assert ingest.Columns({"a": 1}).bounds == {}


def test_ingest_ownership_rule_gives_every_row_one_writer():
    """The rule k_ing_front (csrc/anirec_ingest.hip) decides ownership by, restated in NumPy: the table is cut into chunks
    of 8 192 rows; reach(end) = rows the last user of the chunk ending at `end` continues past it (0 if that user
    started before the chunk or continues for 4 096 rows or more); a user is OWNED by the chunk its first row lies in
    if its last row lies before that chunk's end + reach.  A workgroup writes the flags of its chunk's rows except
    those whose user the left neighbour owns, plus the rows behind its chunk (up to its reach) whose user it owns.
    For any row order every row must have exactly one writer, and every row of an owned user the same one."""
    chunk, ext = 8192, 4096
    rng = np.random.default_rng(3)

    def check(users):
        n = len(users)
        ids = np.unique(users[users >= 0])
        first = {u: int(np.flatnonzero(users == u)[0]) for u in ids}
        last = {u: int(np.flatnonzero(users == u)[-1]) for u in ids}

        def reach(end):
            if end <= 0 or end >= n or users[end - 1] < 0:
                return 0
            u = users[end - 1]
            return last[u] - end + 1 if first[u] >= end - chunk and end <= last[u] < end + ext else 0

        def owns(j, u):
            base = j * chunk
            return base <= first[u] < base + chunk and last[u] < base + chunk + reach(base + chunk)

        writers = np.zeros(n, dtype=int)
        owner_of_row = np.full(n, -1)
        for j in range((n + chunk - 1) // chunk):
            base = j * chunk
            for r in range(base, min(n, base + chunk)):
                u = users[r]
                if u >= 0 and j > 0 and owns(j - 1, u):
                    continue                       # the left neighbour reads on to this row
                writers[r] += 1
                owner_of_row[r] = j if (u >= 0 and owns(j, u)) else -2     # -2: its user is nobody's (the list)
            for r in range(base + chunk, min(n, base + chunk + reach(base + chunk))):
                if users[r] >= 0 and owns(j, users[r]):
                    writers[r] += 1
                    owner_of_row[r] = j
        assert (writers == 1).all(), np.flatnonzero(writers != 1)[:10]
        for u in ids:
            rows = np.flatnonzero(users == u)
            assert len(set(owner_of_row[rows])) == 1, u       # owned whole by one workgroup, or nobody's everywhere

    def blocks(lengths):
        return np.repeat(np.arange(len(lengths)), lengths)

    check(blocks([5000, 2492, 700 + 4095, 300, 8192 * 2 + 11, 250, 6000]))        # reach 4 095: owned
    check(blocks([5000, 2492, 700 + 4096, 300, 9000]))                              # reach 4 096: nobody's
    check(blocks([8192, 8192, 1, 8191, 3]))                                          # blocks ending on the boundaries
    u = blocks([3000, 5000, 400, 7900, 300, 8100, 2000])
    u[[8190, 8192, 8600, 16384, 12000, 5]] = [0, 0, 6, 1, 3, 4]                      # single rows of other users
    u[[100, 9000]] = -1                                                              # rows without a valid user id
    check(u)
    check(rng.integers(0, 40, 30000))                                                # random order: nobody owns anybody
    mix = np.concatenate([blocks([4000, 6000, 300]), rng.integers(0, 5, 2000), blocks([9000, 50]) + 10])
    check(mix)


def test_shuffle_order_equals_pandas_sample():
    df = pd.DataFrame({"a": np.arange(1000)})
    assert (df.sample(frac=1, random_state=42)["a"].to_numpy() == data.shuffle_order(1000, 42)).all()
    assert (orc.shuffle_rows(1000, 42) == data.shuffle_order(1000, 42)).all()


def test_synthetic_dataset_schema_and_split(tmp_path):
    paths = data.write_synthetic_dataset(str(tmp_path), n_users=60, n_anime=200, n_ratings=3000, seed=1)
    df = pd.read_parquet(paths["user_stats"])
    assert list(df.columns) == ["user_id", "anime_id", "rating", "watching_status", "watched_episodes"]
    assert df.rating.between(0, 1).all() and not df.duplicated(["user_id", "anime_id"]).any()
    t = data.load_user_stats(paths["user_stats"])
    assert t.n_users == df.user_id.nunique() and t.n_anime == df.anime_id.nunique()
    tr, te = t.split(100)
    assert te.stop - te.start == 100 and tr.stop == len(t) - 100
    # decoded ids round-trip
    order = data.shuffle_order(len(df), 42)
    assert (t.user_ids[t.user] == df.user_id.to_numpy()[order]).all()
    anime = pd.read_csv(paths["all_anime"])
    assert {"MAL_ID", "Name", "Score", "Genres", "Type", "Episodes", "Japanese name"} <= set(anime.columns)


def test_artifact_store_versions(tmp_path, monkeypatch):
    monkeypatch.setenv("ANIREC_ARTIFACT_DIR", str(tmp_path / "store"))
    f = tmp_path / "x.csv"
    f.write_text("a\n1\n")
    artifacts.log_artifact("x.csv", str(f), "csv")
    f.write_text("a\n2\n")
    artifacts.log_artifact("x.csv", str(f), "csv")
    assert open(artifacts.use_artifact("x.csv:v0")).read() == "a\n1\n"
    assert open(artifacts.use_artifact("x.csv:latest")).read() == "a\n2\n"
    assert open(artifacts.use_artifact("x.csv")).read() == "a\n2\n"
    assert artifacts.use_artifact(str(f)) == str(f)
    with pytest.raises(FileNotFoundError):
        artifacts.use_artifact("nope:latest")


def test_model_container_roundtrip(tmp_path):
    U = np.random.default_rng(0).normal(size=(5, 128)).astype(np.float32)
    A = np.random.default_rng(1).normal(size=(4, 128)).astype(np.float32)
    head = dict(w=1.3, b=0.1, gamma=0.9, beta=-0.2, mov_mean=0.05, mov_var=0.4)
    p = weights_io.save_model(str(tmp_path / "m.safetensors"), U, A, head, [9, 8, 7, 6, 5], [1, 2, 3, 4])
    m = weights_io.load_model(p)
    assert (m["U"] == U).all() and (m["A"] == A).all() and list(m["anime_ids"]) == [1, 2, 3, 4]
    assert all(abs(m["head"][k] - head[k]) < 1e-7 for k in head)
    with pytest.raises(KeyError):
        weights_io.load_model(p, user_name="nope")


@pytest.mark.parametrize("comp", ["neural_network", "similar_anime", "similar_users", "model_recs", "preprocess"])
def test_component_flag_surface_matches_reference(comp, golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "component_flags.json")))[comp]
    mod = load_component(comp)
    assert sorted(mod.STR_FLAGS + mod.BOOL_FLAGS) == sorted(ref["flags"])
    assert sorted(mod.BOOL_FLAGS) == sorted(ref["bool_flags"])
    # every flag is required, strings stay strings, booleans parse like strtobool
    parser = C.make_parser("t", mod.STR_FLAGS, mod.BOOL_FLAGS)
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    for f in mod.BOOL_FLAGS:
        argv += ["--" + f, "True"]
    ns = parser.parse_args(argv)
    assert all(getattr(ns, f) == "x" for f in mod.STR_FLAGS) and all(getattr(ns, f) is True for f in mod.BOOL_FLAGS)
    with pytest.raises(SystemExit):
        parser.parse_args(argv[2:])
    # MLproject: entry point main, same parameters, all typed str
    ml = open(os.path.join(ROOT, comp, "MLproject")).read()
    assert "entry_points:\n  main:" in ml and ml.count("type: str") == len(ref["mlproject_parameters"])
    for f in ref["mlproject_parameters"]:
        assert "--%s {%s}" % (f, f) in ml


def test_clean_and_filters():
    assert C.clean("Yuu☆Yuu☆Hakusho!") == "yuuyuuhakusho"
    assert C.clean("Silent Möbius") == "silentmobius"
    assert C.clean(["SLiceOF life", "va#mpire", None]) == ["sliceoflife", "vampire", "none"]
    g = pd.Series(["Action, Slice of Life", "Vampire, Horror", "Comedy", np.nan])
    assert list(C.genre_mask(g, [None, "SLiceOF life", "va#mpire"])) == [True, True, False, False]
    assert C.str2bool("True") and not C.str2bool("false")
    with pytest.raises(ValueError):
        C.check_types(["TV", "Radio"])


class _OracleEngine:
    """Test double with TrainEngine's interface, backed by the NumPy oracle (tests only)."""

    def __init__(self, n_u, n_a, l2):
        import torch
        self.device = torch.device("cpu")
        self.l2 = l2
        self.n_u, self.n_a = n_u, n_a
        self.state = None
        self.acc = [0.0, 0.0, 0.0]

    def set_head(self, w=1.0, **kw):
        self.w0 = w

    def set_weights(self, U, A):
        self.state = orc.new_state(np.asarray(U), np.asarray(A), orc.new_head(w=self.w0))

    def reset_optimizer(self):
        pass

    def set_epoch(self, u, a, t, starts, counts, alphas):
        self.ep = (np.asarray(u), np.asarray(a), np.asarray(t), starts, counts, alphas)

    def reset_metrics(self):
        self.acc = [0.0, 0.0, 0.0]

    def run(self, n_steps, use_graph=True):
        u, a, t, starts, counts, alphas = self.ep
        for s, c, al in zip(starts, counts, alphas):
            # drive the oracle with the host's alpha: recover lr from alpha and t
            self.state["t"] += 1
            f, g, met = orc.grads(self.state["U"], self.state["A"], u[s:s + c], a[s:s + c], t[s:s + c],
                                  self.state["head"], self.l2)
            orc.adam_update(self.state["U"], self.state["mU"], self.state["vU"], g["U"], al)
            orc.adam_update(self.state["A"], self.state["mA"], self.state["vA"], g["A"], al)
            self.acc[0] += float(met["loss"]) * c
            self.acc[1] += float(met["mse"]) * c
            self.acc[2] += c

    def epoch_metrics(self):
        return self.acc[0] / self.acc[2], self.acc[1] / self.acc[2]

    def evaluate(self, u, a, t):
        ev = orc.evaluate(self.state, np.asarray(u), np.asarray(a), np.asarray(t), self.l2)
        return float(ev["val_loss"]), float(ev["val_mse"])

    def read_state(self):
        return {k: self.state["head"][k] for k in ("w", "b", "gamma", "beta", "mov_mean", "mov_var")}

    def synchronize(self):
        pass

    @property
    def U(self):
        import torch
        return torch.from_numpy(self.state["U"])

    @property
    def A(self):
        import torch
        return torch.from_numpy(self.state["A"])


def test_fit_driver_history_checkpoint_and_early_stopping(monkeypatch):
    import torch
    from anime_recommendations_amd import ops
    # CPU stand-in for the HIP epoch gather (the driver logic is what is under test here)
    monkeypatch.setattr(ops, "gather_ratings", lambda u, a, t, perm: (u[perm], a[perm], t[perm]))
    df = data.synth_user_stats(n_users=40, n_anime=60, n_ratings=1500, seed=3)
    table = data.encode_frame(df)
    cfg = trainer.FitConfig(epochs=6, batch_size=256, test_size=200, verbose=0, seed=5)
    eng = _OracleEngine(table.n_users, table.n_anime, cfg.l2_reg_factor)
    res = trainer.fit(table, cfg, engine=eng)
    h = res.history
    assert list(trainer.history_frame(h).columns) == ["loss", "mse", "val_loss", "val_mse", "lr"]
    n_ep = len(h["loss"])
    assert n_ep == (res.stopped_epoch + 1 if res.stopped_epoch >= 0 else 6)
    assert h["lr"] == [float(np.float32(cfg.lr(e))) for e in range(n_ep)]
    assert res.best_epoch == int(np.argmin(h["val_loss"]))
    if res.stopped_epoch >= 0:
        assert res.stopped_epoch - res.best_epoch == cfg.patience
    assert np.isfinite(res.U).all() and res.best_U is not None
    # early stopping: a monitor that never improves after epoch 0 stops after `patience` more epochs
    seq = iter([(1.0, .1), (2.0, .1), (3.0, .1), (4.0, .1), (5.0, .1), (6.0, .1)])
    eng2 = _OracleEngine(table.n_users, table.n_anime, cfg.l2_reg_factor)
    monkeypatch.setattr(eng2, "evaluate", lambda u, a, t: next(seq))
    res2 = trainer.fit(table, cfg, engine=eng2)
    assert len(res2.history["val_loss"]) == 4 and res2.stopped_epoch == 3 and res2.best_epoch == 0
    assert (res2.U == res2.best_U).all()          # restore_best_weights


def test_init_weights_follow_keras_initialisers():
    U, A, w = trainer.init_weights(1000, 500, 128, seed=1)
    assert U.dtype == np.float32 and abs(U).max() <= 0.05 and abs(U.mean()) < 1e-3
    std = np.sqrt(2.0) / 0.87962566103423978
    assert abs(w) <= 2 * std
