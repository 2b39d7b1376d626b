"""Golden vectors for the user_prefs and user_recs components, produced by the reference's OWN function bodies.

    python tests/golden/make_user_component_fixtures.py <reference checkout>

Uses ``load_functions`` of make_reference_function_fixtures.py (only the listed ``FunctionDef`` nodes of a reference
file are compiled; no module-level statement runs, no reference source text is written).  Functions executed, on
seeded inputs, inside a temporary directory (get_fave_df writes its CSV there):
  user_prefs/user_prefs.py: fave_genres, fave_sources, get_genres, get_sources, get_fave_df  -> ref_fn/user_prefs.json
  user_recs/user_recs.py: similar_user_recs with fave_genres, fave_sources, get_fave_df, get_anime_frame,
      get_sypnopsis, by_genre, clean, get_genres bound from the same file, ID_spec_genres False and True
                                                                                        -> ref_fn/user_recs.json
Also written: user_component_flags.json (argparse flags + MLproject parameters of both components, the extraction
of component_flags.json) and user_component_formats.json (header and row count of the reference's example
figure_file/User_ID_153695_user_prefs.csv and User_ID_153695_user_recs.csv).
"""
import csv
import json
import os
import re
import sys
import tempfile
import types
import warnings
from collections import defaultdict

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_reference_function_fixtures as mrf  # noqa: E402

GOLDEN = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(GOLDEN, "ref_fn")
GENRES = ["Action", "Comedy", "Drama", "Slice of Life", "Sci-Fi", "Romance", "Super Power", "Mystery"]
SOURCES = ["Manga", "Original", "Light novel", "Game", "Visual novel"]


def inputs(seed):
    """Ratings of 30 users over 120 anime ids (10 of them missing from the anime frame), the anime frame in a
    shuffled order, a synopsis frame lacking some anime."""
    rng = np.random.default_rng(seed)
    ids = np.arange(1, 121) * 4
    known = ids[:110]
    cells = []
    for i in range(len(known)):
        k = int(rng.integers(0, 4))
        cell = ", ".join(rng.choice(GENRES, k, replace=False)) if k else np.nan
        cells.append(cell)
    anime_df = pd.DataFrame({
        "anime_id": known, "eng_version": ["Title %03d" % i for i in known], "Name": ["Title %03d" % i for i in known],
        "Genres": cells, "Source": [s if rng.random() > 0.1 else np.nan for s in rng.choice(SOURCES, len(known))],
        "japanese_name": ["J%03d" % i for i in known], "Episodes": rng.integers(1, 50, len(known)),
        "Premiered": "Spring 2010", "Studios": "Studio A", "Score": np.round(rng.uniform(5, 9, len(known)), 2),
        "Type": rng.choice(["TV", "Movie"], len(known))})
    anime_df = anime_df.iloc[rng.permutation(len(anime_df))]
    anime_df.index = np.arange(len(anime_df)) * 3 + 7        # a non-trivial index: the prefs CSV keeps it
    syn = pd.DataFrame({"MAL_ID": known[::2], "Name": ["Title %03d" % i for i in known[::2]],
                        "sypnopsis": ["Synopsis %d" % i for i in known[::2]]})
    rows = []
    for u in range(30):
        k = int(rng.integers(5, 60))
        pop = 1.0 / np.arange(1, len(ids) + 1) ** 0.7
        a = rng.choice(ids, k, replace=False, p=pop / pop.sum())
        r = rng.integers(0, 11, k).astype(np.float64) / 10.0
        for ai, ri in zip(a, r):
            rows.append((100 + u, int(ai), float(ri)))
    df = pd.DataFrame(rows, columns=["user_id", "anime_id", "rating"])
    return df, anime_df, syn


def frame_json(df):
    return {"index": [int(i) for i in df.index], "columns": list(df.columns),
            "rows": [[None if (isinstance(v, float) and np.isnan(v)) else (v.item() if hasattr(v, "item") else v)
                      for v in row] for row in df.itertuples(index=False)]}


def gen_user_prefs():
    df, anime_df, _ = inputs(61)
    cases = []
    for pct in ("80", "50", "95"):
        args = types.SimpleNamespace(favorite_percentile=pct, prefs_csv="user_prefs.csv")
        ns = mrf.load_functions("user_prefs/user_prefs.py",
                                ["fave_genres", "fave_sources", "get_genres", "get_sources", "get_fave_df"], args,
                                {"defaultdict": defaultdict})
        for u in (100, 103, 111, 117, 129):
            g = ns["fave_genres"](u, df, anime_df)
            s = ns["fave_sources"](u, df, anime_df)
            _, gd = ns["get_genres"](g)
            _, sd = ns["get_sources"](s)
            fave, fn = ns["get_fave_df"](g, s, u)
            cases.append({"percentile": float(pct), "user": u, "genre_freq": dict(gd), "source_freq": dict(sd),
                          "fave_df": frame_json(fave), "filename": fn})
    return {"ratings": {c: df[c].tolist() for c in df.columns}, "anime_df": frame_json(anime_df), "cases": cases}


def gen_user_recs():
    df, anime_df, syn = inputs(67)
    helpers = ["similar_user_recs", "fave_genres", "fave_sources", "get_fave_df", "get_anime_frame", "get_sypnopsis",
               "by_genre", "clean", "get_genres"]
    cases = []
    rng = np.random.default_rng(5)
    for spec in (False, True):
        for qi, user in enumerate((101, 108, 122)):
            others = [u for u in range(100, 130) if u != user]
            sims = [int(x) for x in rng.choice(others, 10 + 3 * qi, replace=False)]
            args = types.SimpleNamespace(user_recs_fn="user_recs.csv", ID_spec_genres=spec,
                                         ID_rec_genres='["Action", "Slice of Life", "Mystery"]')
            ns = mrf.load_functions("user_recs/user_recs.py", helpers, args, {"defaultdict": defaultdict})
            pref = ns["get_fave_df"](ns["fave_genres"](user, df, anime_df), ns["fave_sources"](user, df, anime_df))
            sim_df = pd.DataFrame({"similar_users": sims, "similarity": np.linspace(0.9, 0.5, len(sims))})
            frame, fn = ns["similar_user_recs"](user, sim_df, syn, df, None, None, anime_df, 1000, None, None, pref)
            cases.append({"ID_spec_genres": spec, "ID_rec_genres": args.ID_rec_genres, "user": user,
                          "similar_users": sims, "user_pref_eng_versions": pref["eng_version"].tolist(),
                          "n": 1000, "filename": fn, "frame": frame_json(frame)})
    return {"ratings": {c: df[c].tolist() for c in df.columns}, "anime_df": frame_json(anime_df),
            "sypnopsis_df": frame_json(syn), "cases": cases}


def gen_flags_and_formats(ref):
    flags = {}
    for c in ("user_prefs", "user_recs"):
        src = open(os.path.join(ref, c, c + ".py")).read()
        found = re.findall(r'add_argument\(\s*"--(\w+)",\s*type=([^,]+),', src)
        ml = open(os.path.join(ref, c, "MLproject")).read()
        params = re.findall(r"^      (\w+):\s*$", ml, flags=re.M)
        flags[c] = {"flags": [n for n, _ in found], "bool_flags": [n for n, t in found if "strtobool" in t],
                    "mlproject_parameters": params}
    json.dump(flags, open(os.path.join(GOLDEN, "user_component_flags.json"), "w"), indent=1)
    fmt = {}
    for name in ("User_ID_153695_user_prefs.csv", "User_ID_153695_user_recs.csv"):
        with open(os.path.join(ref, "figure_file", name), newline="") as f:
            r = list(csv.reader(f))
        fmt[name] = {"columns": r[0], "n_rows": len(r) - 1}
    json.dump(fmt, open(os.path.join(GOLDEN, "user_component_formats.json"), "w"), indent=1)


def main(ref):
    mrf.REF = ref
    os.makedirs(OUT, exist_ok=True)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        os.chdir(tmp)
        try:
            prefs, recs = gen_user_prefs(), gen_user_recs()
        finally:
            os.chdir(here)
    json.dump(prefs, open(os.path.join(OUT, "user_prefs.json"), "w"))
    json.dump(recs, open(os.path.join(OUT, "user_recs.json"), "w"))
    gen_flags_and_formats(ref)
    print("wrote user_prefs.json, user_recs.json, user_component_flags.json, user_component_formats.json")


if __name__ == "__main__":
    main(sys.argv[1])
