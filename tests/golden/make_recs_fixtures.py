"""Golden vectors for similar_anime, model_recs and the training input, produced by the reference's OWN function bodies.

    python tests/golden/make_recs_fixtures.py <reference checkout>

Uses ``load_functions`` of make_reference_function_fixtures.py: only the listed ``FunctionDef`` nodes of a reference
file are compiled, no module-level statement runs, no reference source text is written.  The bodies reach W&B and
Keras only through module-level names, which are bound to stubs through ``extra=``:
  * ``wandb``: ``init().use_artifact(name, type=...).file()`` returns a file written in a temporary directory from
    the seeded frames (the rating parquet, all_anime.csv, synopses.csv);
  * ``get_model``: a two-array holder for ``get_weights`` (as gen_get_weights does);
  * the model handed to ``recommendations``: ``.predict([user_arr, anime_arr])`` is the forward pass in float64 on
    the committed tables and head (normalised dot, Dense(1), BatchNorm in inference mode, activation):
    ``oracle.anirec_oracle.predict_pairs(..., dtype=np.float64, activation=...)``.
Functions executed, on seeded inputs (reference file:line):
  neural_network/neural_network.py:25-63 get_df                                   -> recs.npz get_df_*
  similar_anime/similar_anime.py:25-60 main_df_by_anime, :63-93 get_anime_df (with get_anime_name, clean)
                                                                                  -> recs.npz main_*, recs.json
  similar_anime/similar_anime.py:364-471 anime_recs (with get_sypnopses_df, get_weights, get_types,
      get_anime_frame, get_sypnopsis, by_genre, get_genres, clean, main_df_by_anime from the same file)
                                                                                  -> recs.json similar_anime
  model_recs/model_recs.py:373-456 recommendations (with get_full_df, get_anime_df, get_sypnopses_df, get_sypnopsis,
      by_genre, get_genres, clean; id_anime / unwatched from get_user_anime_arr / get_unwatched; the model stub
      looks the reference's indices up by id, as those number ids in the shuffled frame's order)
                                                                                  -> recs.json model_recs
Next to every listed row the fp64 score is recorded: the fp64 dot of the reference's own normalised rows
(get_weights) for similar_anime, the float64 model stub for model_recs.  recs.npz holds the inputs (ratings,
tables, all_anime.csv and synopses.csv as UTF-8 bytes) and the outputs (the ranked lists and the reference's column
values as a JSON blob); recs.json holds the flags, the case settings and the deviations.  Where a reference body
raises, the exception type is recorded as a deviation instead of an output (recs.json "deviations")."""
import io
import json
import os
import sys
import tempfile
import types
import warnings
import zipfile

import numpy as np
import pandas as pd

GOLDEN = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, GOLDEN)
sys.path.insert(0, ROOT)
import make_reference_function_fixtures as mrf  # noqa: E402
from oracle import anirec_oracle as orc  # noqa: E402

OUT = os.path.join(GOLDEN, "ref_fn")
D = 128
GENRES = ["Action", "Comedy", "Drama", "Slice of Life", "Sci-Fi", "Romance", "Super Power", "Mystery", "Sports"]
TYPES = ["TV", "OVA", "Movie", "Special", "ONA", "Music"]
SA_TYPES = '["Movie", "Special", "ONA"]'
SA_GENRES = '["Action", "Slice of Life", "None"]'
MR_TYPES = '["TV", "Movie"]'
MR_GENRES = '["Comedy", "Mystery", "None"]'
COUNTS = (10, 127, 129, 100000)          # <= 128: the existing kernels; > 128: the *_topk_large kernels; "every row"
HEADS = {
    "sigmoid": dict(w=2.5, b=0.1, gamma=1.2, beta=0.3, mov_mean=0.05, mov_var=0.8),
    "relu": dict(w=3.0, b=-0.2, gamma=1.1, beta=-0.15, mov_mean=0.1, mov_var=0.5),   # ~half the pairs are 0
}
FLAGS = dict(project_name="anime_recommendations", main_df="user_stats.parquet", main_df_type="parquet",
             input_data="user_stats.parquet", anime_df="all_anime.csv", anime_df_type="raw_data",
             sypnopses_df="synopses.csv", sypnopsis_df="synopses.csv", sypnopsis_df_type="raw_data",
             model="wandb_anime_nn.h5", model_type="h5", anime_emb_name="anime_embedding",
             ID_emb_name="user_embedding")


# ---- stubs ------------------------------------------------------------------------------------------------------
class _Artifact:
    def __init__(self, path):
        self._path = path

    def file(self):
        return self._path


class _Run:
    def __init__(self, files):
        self._files = files

    def use_artifact(self, name, type=None):
        return _Artifact(self._files[name])


class WandbStub:
    """``wandb.init(...).use_artifact(name, type=...).file()`` -> the local file logged under ``name``."""

    def __init__(self, files):
        self._files = files

    def init(self, **kw):
        return _Run(self._files)


class ModelStub:
    """``model.predict([user_arr, anime_arr])``: the forward pass in float64 on the committed tables and head."""

    def __init__(self, U, A, head, act, user_rows, anime_rows):
        self.U, self.A, self.head, self.act = U, A, head, act
        self.user_rows, self.anime_rows = user_rows, anime_rows

    def predict(self, id_anime, verbose=0):
        # the caller's indices -> the table rows of the same ids (see run_recommendations)
        ui = self.user_rows[np.asarray(id_anime[0], np.int64)]
        ai = self.anime_rows[np.asarray(id_anime[1], np.int64)]
        p = orc.predict_pairs(self.U, self.A, self.head, ui, ai, dtype=np.float64, activation=self.act)
        return np.asarray(p, np.float64).reshape(-1, 1)


# ---- deterministic writers --------------------------------------------------------------------------------------
def save_npz(path, **arrays):
    """np.savez_compressed with a fixed entry date, so that a rerun writes the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def _bytes(text):
    return np.frombuffer(text.encode("utf-8"), np.uint8)


def _pop(case, *keys):
    return {k: case.pop(k) for k in keys}


def jval(v):
    if v is None or (isinstance(v, float) and np.isnan(v)):
        return None
    if isinstance(v, np.generic):
        v = v.item()
        if isinstance(v, float) and np.isnan(v):
            return None
    return v


# ---- seeded inputs ----------------------------------------------------------------------------------------------
def ratings(rng, user_ids, anime_pool, lo, hi):
    """Rows sorted by user (as preprocess writes them), anime in a random order within a user, each user rating
    between lo and hi distinct anime drawn with a Zipf-like popularity."""
    pop = 1.0 / np.arange(1, len(anime_pool) + 1) ** 0.6
    pop /= pop.sum()
    u, a, r = [], [], []
    for uid in user_ids:
        k = int(rng.integers(lo, hi + 1))
        pick = rng.choice(anime_pool, k, replace=False, p=pop)
        u += [uid] * k
        a += pick.tolist()
        r += (rng.integers(0, 11, k) / 10.0).tolist()
    return pd.DataFrame({"user_id": np.asarray(u, np.int64), "anime_id": np.asarray(a, np.int64),
                         "rating": np.asarray(r, np.float64)})


def anime_tables(rng, ids, names):
    n = len(ids)
    genres = []
    for _ in range(n):
        k = int(rng.integers(1, 4))
        genres.append(", ".join(sorted(rng.choice(GENRES, k, replace=False))))
    score = np.round(rng.uniform(4, 9.5, n), 2).astype(object)
    score[rng.choice(n, 40, replace=False)] = 7.5                # Score ties for the loader's sort
    anime = pd.DataFrame({
        "MAL_ID": ids, "Name": names, "Score": score, "Genres": genres, "English name": names,
        "Japanese name": ["アニメ%05d" % i for i in ids],
        "Type": rng.choice(TYPES, n, p=[0.4, 0.1, 0.2, 0.1, 0.15, 0.05]),
        "Episodes": rng.integers(1, 100, n).astype(str).astype(object),
        "Premiered": rng.choice(["Spring 2010", "Fall 2015", "Winter 2019"], n).astype(object),
        "Studios": rng.choice(["Studio A", "Studio B", "Studio C"], n),
        "Source": rng.choice(["Manga", "Original", "Light novel", "Game"], n),
        "Rating": rng.choice(["PG-13 - Teens 13 or older", "R - 17+ (violence & profanity)", "G - All Ages"], n),
        "Members": rng.integers(100, 2_000_000, n)})
    for col, m in (("Score", 12), ("Episodes", 9), ("Premiered", 30), ("English name", 15), ("Genres", 6)):
        anime.loc[rng.choice(n, m, replace=False), col] = "Unknown"
    anime = anime.iloc[rng.permutation(n)].reset_index(drop=True)
    has_syn = rng.random(n) > 0.12
    syn = pd.DataFrame({"MAL_ID": anime["MAL_ID"][has_syn], "Name": anime["Name"][has_syn],
                        "Score": anime["Score"][has_syn], "Genres": anime["Genres"][has_syn],
                        "sypnopsis": ["Synopsis of anime %d." % i for i in anime["MAL_ID"][has_syn]]})
    syn.loc[syn.index[:3], "sypnopsis"] = np.nan                 # a synopsis row with an empty text
    return anime, syn.reset_index(drop=True)


def tables(rng, n_a, n_u):
    """Clustered tables on a 1/64 grid (they compress), then the rows that make the edges."""
    ca = rng.integers(-40, 41, (10, D))
    A = (ca[rng.integers(0, 10, n_a)] + rng.integers(-48, 49, (n_a, D))).astype(np.float32) / np.float32(64)
    U = (ca[rng.integers(0, 10, n_u)] + rng.integers(-48, 49, (n_u, D))).astype(np.float32) / np.float32(64)
    return A, U


def ranked(A, q, skip=()):
    Wn = orc.rownorm(A).astype(np.float64)
    s = Wn @ Wn[q]
    s[list(skip) + [q]] = -np.inf
    s[np.isnan(s)] = -np.inf
    return np.argsort(-s, kind="stable")


def build_inputs():
    rng = np.random.default_rng(20261016)
    n_pool = 560
    pool = np.sort(rng.choice(np.arange(1, 48000), n_pool, replace=False))
    user_ids = np.sort(rng.choice(np.arange(1, 350000), 14, replace=False))
    df = ratings(rng, user_ids, pool, 400, 420)
    anime_ids = df["anime_id"].unique()                              # get_df / main_df_by_anime index order
    n_a = len(anime_ids)
    extra = np.setdiff1d(np.arange(48000, 48010), anime_ids)[:6]     # in all_anime.csv, rated by nobody
    ids = np.concatenate([np.sort(anime_ids), extra])
    names = ["Title %05d" % i for i in ids]
    pos = {int(a): i for i, a in enumerate(ids)}
    # queries: an exact Name; a name found only through the cleaned-name fallback; a name whose cleaned form is
    # another anime's Name (the reference's first lookup is Name == clean(query))
    qa, qb, qc, qc2 = (int(anime_ids[i]) for i in (17, 230, 301, 402))
    names[pos[qa]] = "Kaguya-sama: Love is War"
    names[pos[qb]] = "Steins;Gate 0"
    names[pos[qc]] = "Re:Zero"
    names[pos[qc2]] = "rezero"
    anime, syn = anime_tables(rng, ids, names)
    A, U = tables(rng, n_a, len(user_ids))
    idx_of = {int(a): i for i, a in enumerate(anime_ids)}
    zero = idx_of[int(anime_ids[5])]
    A[zero] = 0.0                                                    # zero row: NaN similarities
    q = idx_of[qa]
    # exact duplicate rows whose ties straddle the cuts at 10 and 127 of the unfiltered ranking of query qa
    used = {q, zero} | {idx_of[a] for a in (qb, qc, qc2)}
    for cut in (10, 40, 127, 129):          # ascending: a later pair never shifts an earlier one
        order = [int(i) for i in ranked(A, q, [zero])]
        src = order[cut - 1]
        dst = next(i for i in order[::-1] if i not in used and i != src)
        A[dst] = A[src]
        used |= {src, dst}
    dups = sorted(used - {q, zero} - {idx_of[a] for a in (qb, qc, qc2)})
    return dict(df=df, anime=anime, syn=syn, A=A, U=U, anime_ids=anime_ids, user_ids=user_ids, zero=zero,
                dups=dups, queries={"exact": "Kaguya-sama: Love is War", "fallback": "STEINS GATE 0!",
                                    "cleaned_name_first": "Re:Zero"})


def write_inputs(tmp, df, anime, syn):
    files = {FLAGS["main_df"]: os.path.join(tmp, "user_stats.parquet"),
             FLAGS["anime_df"]: os.path.join(tmp, "all_anime.csv"),
             FLAGS["sypnopses_df"]: os.path.join(tmp, "synopses.csv")}
    df.to_parquet(files[FLAGS["main_df"]], index=False)
    anime.to_csv(files[FLAGS["anime_df"]], index=False)
    syn.to_csv(files[FLAGS["sypnopses_df"]], index=False)
    return files


# ---- the reference runs -----------------------------------------------------------------------------------------
def ns_for(relpath, names, files, **flags):
    args = types.SimpleNamespace(**dict(FLAGS, **flags))
    return mrf.load_functions(relpath, names, args, {"wandb": WandbStub(files)})


def run_get_df(files):
    ns = ns_for("neural_network/neural_network.py", ["get_df"], files)
    out, n_u, n_a = ns["get_df"]()
    return out, n_u, n_a


def run_main_df_by_anime(files):
    ns = ns_for("similar_anime/similar_anime.py", ["main_df_by_anime"], files)
    return ns["main_df_by_anime"]()


SA_HELPERS = ["anime_recs", "get_sypnopses_df", "get_weights", "main_df_by_anime", "get_types", "clean",
              "get_anime_frame", "get_sypnopsis", "by_genre", "get_genres", "get_anime_df", "get_anime_name"]
MR_HELPERS = ["recommendations", "get_full_df", "get_anime_df", "get_anime_name", "get_sypnopses_df", "get_sypnopsis",
              "by_genre", "get_genres", "clean", "get_unwatched", "get_user_anime_arr"]


def _holder(A, U):
    return mrf._TwoTables({FLAGS["anime_emb_name"]: A, FLAGS["ID_emb_name"]: U})


def run_anime_recs(files, A, U, query, count, spec_types, spec_genres):
    ns = ns_for("similar_anime/similar_anime.py", SA_HELPERS, files, types=SA_TYPES, spec_types=spec_types,
                anime_rec_genres=SA_GENRES, an_spec_genres=spec_genres)
    ns["get_model"] = lambda: _holder(A, U)
    anime_df = ns["get_anime_df"]()
    try:
        frame, fn, translated = ns["anime_recs"](query, count, anime_df)
    except Exception as e:                                # noqa: BLE001  (recorded, not mirrored)
        return None, type(e).__name__
    return (frame, fn, translated), None


def _rows_by_id(order, trained):
    row = {int(x): i for i, x in enumerate(trained)}
    return np.asarray([row[int(x)] for x in order], np.int64)


def run_recommendations(files, A, U, head, act, user, n_recs, spec_types, spec_genres, types_list=MR_TYPES):
    ns = ns_for("model_recs/model_recs.py", MR_HELPERS, files, specify_types=spec_types, anime_types=types_list,
                specify_genres=spec_genres, model_genres=MR_GENRES)
    raw = pd.read_parquet(files[FLAGS["main_df"]])
    users_trained, anime_trained = raw["user_id"].unique(), raw["anime_id"].unique()      # get_df's encoding
    df = ns["get_full_df"]()
    anime_df = ns["get_anime_df"]()
    syp = ns["get_sypnopses_df"]()
    unwatched = ns["get_unwatched"](df, anime_df, user)
    arr = ns["get_user_anime_arr"](df, anime_df, user, unwatched)
    # recommendations, get_unwatched and get_user_anime_arr number ids by first appearance in get_full_df's SHUFFLED
    # frame, the model's rows follow get_df's order before the shuffle: the stub looks each index up by its id, so
    # that a prediction belongs to the (user, anime) the reference names (recs.json deviations
    # "model_recs_shuffled_encoding")
    user_rows, anime_rows = _rows_by_id(df["user_id"].unique(), users_trained), _rows_by_id(df["anime_id"].unique(),
                                                                                          anime_trained)
    model = ModelStub(U, A, head, act, user_rows, anime_rows)
    try:
        return ns["recommendations"](df, anime_df, syp, model, arr, unwatched, n_recs), None
    except Exception as e:                                # noqa: BLE001
        return None, type(e).__name__


def cosine64(A, ids_by_index, q):
    ns = mrf.load_functions("similar_anime/similar_anime.py", ["get_weights"],
                            types.SimpleNamespace(**FLAGS))
    with np.errstate(all="ignore"):
        Wn, _ = ns["get_weights"](_holder(A, A[:1]))
    Wn = Wn.astype(np.float64)
    return Wn @ Wn[q]


def frame_rows(frame, key, rows):
    """The non-score columns of every listed row, once per key (asserted equal wherever a key recurs):
    rows = {"columns": [...], "data": {key: [value per column]}}."""
    cols = [c for c in frame.columns if c not in ("Similarity", "Prediction", key)]
    if "columns" not in rows:
        rows.update(columns=cols, data={})
    assert rows["columns"] == cols, (rows["columns"], cols)
    for _, r in frame.iterrows():
        k = str(jval(r[key]))
        vals = [jval(r[c]) for c in cols]
        assert rows["data"].setdefault(k, vals) == vals, (k, rows["data"][k], vals)


def gen_similar_anime(inp, files):
    A, U, anime_ids = inp["A"], inp["U"], inp["anime_ids"]
    anime = inp["anime"]
    name_to_id = dict(zip(anime["Name"], anime["MAL_ID"]))
    idx_of = {int(a): i for i, a in enumerate(anime_ids)}
    cases, rows = [], {}
    plan = [("exact", t, g, c) for t in (False, True) for g in (False, True) for c in COUNTS]
    plan += [("fallback", t, g, c) for t in (False, True) for g in (False, True) for c in COUNTS]
    plan += [("cleaned_name_first", False, False, c) for c in (10, 100000)]
    for qkey, spec_t, spec_g, count in plan:
        query = inp["queries"][qkey]
        res, err = run_anime_recs(files, A, U, query, count, spec_t, spec_g)
        assert err is None, (qkey, spec_t, spec_g, count, err)
        frame, fn, translated = res
        # the anime the reference resolved the query to: the one absent from its own (all-rows) output
        ids = [int(name_to_id[n]) for n in frame["Name"]]
        cases.append(dict(query_key=qkey, query=query, spec_types=spec_t, spec_genres=spec_g, count=count,
                          filename=fn, translated=translated, columns=list(frame.columns),
                          anime_id=ids))
        frame_rows(frame.assign(anime_id=ids), "anime_id", rows)
    # the resolved query of each case: the row missing from the unfiltered all-rows output
    all_rows = set(int(a) for a in anime_ids)
    for c in cases:
        full = next(d for d in cases if d["query_key"] == c["query_key"] and not d["spec_types"]
                    and not d["spec_genres"] and d["count"] == 100000)
        (c["query_id"],) = all_rows - set(full["anime_id"])
        cos = cosine64(A, anime_ids, idx_of[c["query_id"]])
        c["cos64"] = [jval(float(cos[idx_of[a]])) for a in c["anime_id"]]
    return cases, rows


def gen_model_recs(inp, files):
    A, U, user_ids = inp["A"], inp["U"], inp["user_ids"]
    cases, rows = [], {}
    for user in (int(user_ids[3]), int(user_ids[11])):
        for act, head in HEADS.items():
            h = orc.new_head(**head)
            for spec_t in (False, True):
                for spec_g in (False, True):
                    for n in COUNTS:
                        frame, err = run_recommendations(files, A, U, h, act, user, n, spec_t, spec_g)
                        case = dict(user=user, activation=act, spec_types=spec_t, spec_genres=spec_g, n_recs=n,
                                    reference_error=err)
                        if err is not None:
                            frame = pinned_model_recs(files, A, U, h, act, user, n, spec_t, spec_g)
                        case.update(columns=list(frame.columns), anime_id=[int(a) for a in frame["anime_id"]],
                                    prediction=[jval(float(x)) for x in frame["Prediction"]])
                        frame_rows(frame, "anime_id", rows)
                        cases.append(case)
    return cases, rows


def pinned_model_recs(files, A, U, h, act, user, n, spec_t, spec_g):
    """What a case the reference cannot run is held to:
    specify_types False — the reference names its score column 'Prediciton_rating' and then sorts by 'Prediction'
    (KeyError); without a Type filter every unwatched anime is kept, which is the reference's own run with all six
    types allowed (every fixture anime has a Type).
    specify_genres True — the reference compares clean()ed genres with the raw Genres text, matches nothing and
    sorts None (AttributeError); the build filters by similar_anime's by_genre, so the pinned frame is the
    reference's own similar_anime.by_genre applied to its genre-free frame, sorted, cut at n."""
    frame, err = run_recommendations(files, A, U, h, act, user, 100000, True, False,
                                     types_list=MR_TYPES if spec_t else str(TYPES))
    assert err is None, err
    if spec_g:
        ns = mrf.load_functions("similar_anime/similar_anime.py", ["by_genre", "get_genres", "clean"],
                                types.SimpleNamespace(anime_rec_genres=MR_GENRES))
        frame = ns["by_genre"](frame)
    return frame.sort_values(by="Prediction", ascending=False)[:n]


def gen_deviations(inp, files, files_mr, tmp):
    A, U = inp["A"], inp["U"]
    dev = {}
    # similar_anime: an embedded anime without an all_anime.csv row -> IndexError in the per-row lookup
    no_meta = int(inp["anime_ids"][40])
    d = os.path.join(tmp, "nometa")
    os.makedirs(d)
    f2 = write_inputs(d, inp["df"], inp["anime"][inp["anime"].MAL_ID != no_meta], inp["syn"])
    _, err = run_anime_recs(f2, A, U, inp["queries"]["exact"], 10, False, False)
    dev["similar_anime_no_metadata"] = dict(anime_id=no_meta, reference_error=err)
    # model_recs: the reference cannot run without a Type filter, nor with a Genre filter
    h = orc.new_head(**HEADS["sigmoid"])
    user = int(inp["user_ids"][3])
    _, e1 = run_recommendations(files_mr, A, U, h, "sigmoid", user, 10, False, False)
    _, e2 = run_recommendations(files_mr, A, U, h, "sigmoid", user, 10, True, True)
    ns = ns_for("model_recs/model_recs.py", ["get_full_df"], files_mr)
    shuffled = ns["get_full_df"]()
    raw = pd.read_parquet(files_mr[FLAGS["main_df"]])
    dev["model_recs_shuffled_encoding"] = dict(
        note="recommendations / get_unwatched / get_user_anime_arr number ids in get_full_df's shuffled order; "
             "the model's rows are in get_df's order",
        anime_orders_agree=bool(np.array_equal(shuffled["anime_id"].unique(), raw["anime_id"].unique())),
        user_orders_agree=bool(np.array_equal(shuffled["user_id"].unique(), raw["user_id"].unique())))
    dev["model_recs_specify_types_false"] = dict(reference_error=e1)
    dev["model_recs_specify_genres_true"] = dict(reference_error=e2)
    return dev


def gen_min_ratings(tmp):
    """A frame where users below 400 ratings come first: get_df and main_df_by_anime encode anime differently."""
    rng = np.random.default_rng(7)
    pool = np.arange(1, 601) * 3
    small = ratings(rng, [5, 9], pool[::-1], 20, 30)
    big = ratings(rng, [11, 12, 20], pool, 400, 410)
    df = pd.concat([small, big], ignore_index=True)
    d = os.path.join(tmp, "minr")
    os.makedirs(d)
    files = write_inputs(d, df, pd.DataFrame({"MAL_ID": [1]}), pd.DataFrame({"MAL_ID": [1]}))
    g, _, _ = run_get_df(files)
    m, a2i, i2a = run_main_df_by_anime(files)
    return df, g, m, i2a


def main(ref):
    mrf.REF = ref
    inp = build_inputs()
    no_meta = [int(inp["anime_ids"][i]) for i in (60, 61, 62, 63, 64)]
    arrays = {"ratings_user_id": inp["df"]["user_id"].to_numpy(), "ratings_anime_id": inp["df"]["anime_id"].to_numpy(),
              "ratings_rating": inp["df"]["rating"].to_numpy(), "A": inp["A"], "U": inp["U"]}
    with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        files = write_inputs(tmp, inp["df"], inp["anime"], inp["syn"])
        g, n_u, n_a = run_get_df(files)
        arrays.update(get_df_index=g.index.to_numpy(np.int64), get_df_user=g["user"].to_numpy(np.int64),
                      get_df_anime=g["anime"].to_numpy(np.int64), get_df_rating=g["rating"].to_numpy())
        m, a2i, i2a = run_main_df_by_anime(files)
        assert m.columns.tolist() == ["user", "anime", "rating", "user_id", "anime_id"]
        arrays.update(main_index=m.index.to_numpy(np.int64), main_user=m["user"].to_numpy(np.int64),
                      main_anime=m["anime"].to_numpy(np.int64), main_rating=m["rating"].to_numpy(),
                      main_index_to_anime=np.asarray([i2a[i] for i in range(len(i2a))], np.int64))
        assert np.array_equal(arrays["main_index_to_anime"], inp["anime_ids"])
        ns = ns_for("similar_anime/similar_anime.py", ["get_anime_df", "get_anime_name", "clean"], files)
        adf = ns["get_anime_df"]()
        sa_cases, sa_rows = gen_similar_anime(inp, files)
        # model_recs sees five rated anime without an all_anime.csv row (the reference skips them)
        d = os.path.join(tmp, "mr")
        os.makedirs(d)
        files_mr = write_inputs(d, inp["df"], inp["anime"][~inp["anime"].MAL_ID.isin(no_meta)], inp["syn"])
        mr_cases, mr_rows = gen_model_recs(inp, files_mr)
        deviations = gen_deviations(inp, files, files_mr, tmp)
        mdf, mg, mm, mi2a = gen_min_ratings(tmp)
    arrays.update(minr_user_id=mdf["user_id"].to_numpy(), minr_anime_id=mdf["anime_id"].to_numpy(),
                  minr_rating=mdf["rating"].to_numpy(), minr_get_df_anime=mg["anime"].to_numpy(np.int64),
                  minr_get_df_index=mg.index.to_numpy(np.int64), minr_main_anime=mm["anime"].to_numpy(np.int64),
                  minr_main_user=mm["user"].to_numpy(np.int64), minr_main_index=mm.index.to_numpy(np.int64),
                  minr_main_index_to_anime=np.asarray([mi2a[i] for i in range(len(mi2a))], np.int64))
    deviations["main_df_by_anime_min_ratings"] = dict(
        note="users below 400 ratings change the anime encoding of main_df_by_anime against get_df's",
        encodings_agree=bool(np.array_equal(mg.loc[mm.index, "anime"].to_numpy(), mm["anime"].to_numpy())))
    # the ranked lists, the reference's column values and the two CSV inputs travel in recs.npz (as UTF-8 bytes);
    # recs.json keeps what a reader checks by eye: flags, case settings, deviations
    lists = {"similar_anime": [_pop(c, "anime_id", "cos64") for c in sa_cases], "similar_anime_rows": sa_rows,
             "model_recs": [_pop(c, "anime_id", "prediction") for c in mr_cases], "model_recs_rows": mr_rows,
             "get_anime_df": {"anime_id": [int(a) for a in adf["anime_id"]], "eng_version": list(adf["eng_version"]),
                              "Score": [jval(s) for s in adf["Score"]]}}
    arrays.update(lists_json=_bytes(json.dumps(lists, ensure_ascii=False, separators=(",", ":"))),
                  anime_csv=_bytes(inp["anime"].to_csv(index=False)), synopses_csv=_bytes(inp["syn"].to_csv(index=False)))
    save_npz(os.path.join(OUT, "recs.npz"), **arrays)
    rec = {"flags": dict(SA_TYPES=SA_TYPES, SA_GENRES=SA_GENRES, MR_TYPES=MR_TYPES, MR_GENRES=MR_GENRES),
           "counts": list(COUNTS), "zero_row": int(inp["zero"]), "duplicate_rows": [int(i) for i in inp["dups"]],
           "get_df": {"n_users": int(n_u), "n_anime": int(n_a), "columns": list(g.columns)},
           "main_df_by_anime": {"columns": list(m.columns)},
           "get_anime_df": {"columns": list(adf.columns)},
           "similar_anime": {"cases": sa_cases},
           "model_recs": {"users_embedded": [int(u) for u in inp["user_ids"]], "heads": HEADS, "cases": mr_cases,
                          "no_metadata": no_meta},
           "deviations": deviations}
    for part in ("similar_anime", "model_recs"):         # every case lists the same columns: recorded once
        cols = {tuple(c.pop("columns")) for c in rec[part]["cases"]}
        assert len(cols) == 1, cols
        rec[part]["columns"] = list(cols.pop())
    with open(os.path.join(OUT, "recs.json"), "w", encoding="utf-8") as f:
        json.dump(rec, f, ensure_ascii=False, separators=(",", ":"))
    print("wrote recs.npz, recs.json")


if __name__ == "__main__":
    main(sys.argv[1])
