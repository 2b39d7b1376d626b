#!/usr/bin/env python
"""content_recs component — content-based lists from all_anime.csv's own columns: the anime closest to a query anime, or
one user's list, by TF-IDF vectors of Genres, Type, Source, Studios and Rating (and, opt-in, the synopsis words).  No
model takes part and the listed anime need no rating, so it is the one component that serves a title nobody has rated
yet.  also_liked's data and filter flags, plus

    --user_query <user id | none>        list for this user instead of an anime (default none)
    --content_columns <a,b,...>          columns the vectors are built from (default Genres,Type,Source,Studios,Rating;
                                         Sypnopsis is opt-in)
    --content_weight rating|centered|one how a user's ratings weigh their titles (default rating; centered = the rating
                                         minus the user's mean: a title rated below it pushes away)
    --content_min_rating <0..1>          the scaled rating from which a rating enters the profile (default 0.0)

Exactly one of --anime_query and --user_query (or --random_anime) names the query.  With an anime the CSV holds
similar_anime's columns (``Similarity`` is the content cosine) and ``Shared_tokens``; with a user, model_recs' columns with
``Content_score`` in the place of the predicted rating.  The profiles and scores run in libanirec (HIP): int64 fixed-point
profile sums, one divide, a fixed fp32 chain per anime, then the exact select."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, cli, components as C  # noqa: E402

STR_FLAGS = ["main_df_type", "anime_df_type", "sypnopsis_df_type", "project_name", "main_df", "sypnopses_df", "anime_df",
             "anime_query", "a_query_number", "anime_rec_genres", "types", "a_rec_type"]
BOOL_FLAGS = ["random_anime", "an_spec_genres", "spec_types", "save_sim_anime"]
OPTIONAL_FLAGS = {"user_query": "none", "content_columns": ",".join(C.CONTENT_COLUMNS), "content_weight": "rating",
                  "content_min_rating": 0.0}
CONTENT_WEIGHTS = ("rating", "centered", "one")     # recs.CONTENT_WEIGHTS, named here so that parsing imports no torch
KNOWN_COLUMNS = C.CONTENT_COLUMNS + ("Sypnopsis",)

logger = C.setup_logging("content_recs")


def user_query(v):
    s = str(v).strip()
    return "none" if s.lower() in ("", "none") else str(int(s))


def content_columns(v):
    cols = [c.strip() for c in str(v).split(",") if c.strip()]
    if not cols or len(set(cols)) != len(cols) or any(c not in KNOWN_COLUMNS for c in cols):
        raise ValueError("%r is not a list of distinct names of %s" % (v, ", ".join(KNOWN_COLUMNS)))
    return ",".join(cols)


def content_weight(v):
    s = str(v).strip().lower()
    if s not in CONTENT_WEIGHTS:
        raise ValueError("%r is not one of %s" % (v, ", ".join(CONTENT_WEIGHTS)))
    return s


def content_min_rating(v):
    x = float(str(v).strip())
    if not 0.0 <= x <= 1.0:
        raise ValueError("%r is not a scaled rating in 0 .. 1" % (v,))
    return x


def make_parser():
    p = C.make_parser("Content-based lists from the anime metadata", STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--user_query", type=user_query, default=OPTIONAL_FLAGS["user_query"])
    p.add_argument("--content_columns", type=content_columns, default=OPTIONAL_FLAGS["content_columns"])
    p.add_argument("--content_weight", type=content_weight, default=OPTIONAL_FLAGS["content_weight"])
    p.add_argument("--content_min_rating", type=content_min_rating, default=OPTIONAL_FLAGS["content_min_rating"])
    return p


def query_of(args):
    """("anime", name | None for a random one) or ("user", id): ValueError unless exactly one query is named."""
    anime = str(args.anime_query).strip()
    has_anime = bool(args.random_anime) or anime.lower() not in ("", "none")
    has_user = args.user_query != "none"
    if has_anime == has_user:
        raise ValueError("content_recs takes exactly one of --anime_query (or --random_anime) and --user_query (got %s)"
                         % ("both" if has_anime else "neither"))
    return ("user", int(args.user_query)) if has_user else ("anime", None if args.random_anime else anime)


def go(args):
    import pandas as pd
    kind, query = query_of(args)
    anime_df = C.load_anime_df(artifacts.use_artifact(args.anime_df, args.anime_df_type))
    syn_df = C.load_synopses(artifacts.use_artifact(args.sypnopses_df, args.sypnopsis_df_type))
    columns = args.content_columns.split(",")
    types = C.literal(args.types) if args.spec_types else None
    genres = C.literal(args.anime_rec_genres) if args.an_spec_genres else None
    meta = {"content_columns": args.content_columns, "content_weight": args.content_weight,
            "content_min_rating": args.content_min_rating}
    if kind == "anime":
        if query is None:
            query = random.choice(anime_df["Name"].dropna().unique().tolist())
            logger.info("Using %s as random input anime", query)
        frame, fn = C.content_similar_frame(anime_df, syn_df, query, int(args.a_query_number), types, genres, columns)
        what = "Anime closest by content to: " + str(query)
        meta.update({"Queried anime": query})
    else:
        main_df = pd.read_parquet(artifacts.use_artifact(args.main_df, args.main_df_type))
        frame = C.content_recs_frame(main_df, anime_df, syn_df, query, int(args.a_query_number), types, genres, columns,
                                     args.content_weight, args.content_min_rating)
        fn = "User_ID_%d_content_recs.csv" % query
        what = "Content-based recommendations for user %d" % query
        meta.update({"Queried user": query, "Main data frame used": args.main_df})
    frame.to_csv(fn, index=False)
    artifacts.log_artifact(fn, fn, args.a_rec_type, what, metadata=dict(meta, Filename=fn))
    if not args.save_sim_anime:
        os.remove(fn)
    return frame


if __name__ == "__main__":
    cli.run("content_recs", logger, go, make_parser())
