#!/usr/bin/env python
"""ease_recs component — lists from EASE (Steck 2019), the closed-form linear item-item model of the liked pairs: the
anime with the largest weights in a query anime's row, or one user's list among the anime they have not rated.  No
neural model takes part; the fit is one fp64 matrix inverse on the GPU.  also_liked's data and filter flags, plus

    --user_query <user id | none>    list for this user instead of an anime (default none)
    --ease_reg <float > 0>           the L2 weight of the fit (default 500, the paper's value for a data set of about
                                     this many users; not tuned on this data)
    --ease_neighbours <K>            K > 0 keeps the K largest weights of every anime only (default 0: the dense model)
    --liked_min_rating <0..1>        the scaled rating from which a rating counts as liked (default 0.0)

Exactly one of --anime_query and --user_query (or --random_anime) names the query.  With an anime the CSV holds
similar_anime's columns (``Similarity`` is the weight W[query, anime]); with a user, model_recs' columns with
``Ease_score`` in the place of the predicted rating.  The counts, the inverse, the weights, the score rows and the
select run in libanirec (HIP): DESIGN.md §4.24."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, cli, components as C  # noqa: E402

STR_FLAGS = ["main_df_type", "anime_df_type", "sypnopsis_df_type", "project_name", "main_df", "sypnopses_df", "anime_df",
             "anime_query", "a_query_number", "anime_rec_genres", "types", "a_rec_type"]
BOOL_FLAGS = ["random_anime", "an_spec_genres", "spec_types", "save_sim_anime"]
OPTIONAL_FLAGS = {"user_query": "none", "ease_reg": cli.EASE_FLAGS["ease_reg"][1],
                  "ease_neighbours": cli.EASE_FLAGS["ease_neighbours"][1], "liked_min_rating": 0.0}

logger = C.setup_logging("ease_recs")


def user_query(v):
    s = str(v).strip()
    return "none" if s.lower() in ("", "none") else str(int(s))


def ease_reg(v):
    x = float(str(v).strip())
    if not 0.0 < x < float("inf"):
        raise ValueError("%r is not a finite weight > 0" % (v,))
    return x


def ease_neighbours(v):
    k = int(str(v).strip())
    if k < 0:
        raise ValueError("%r is not a count >= 0" % (v,))
    return k


def make_parser():
    p = C.make_parser("Lists from the EASE item-item model of the liked pairs", STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--user_query", type=user_query, default=OPTIONAL_FLAGS["user_query"])
    p.add_argument("--ease_reg", type=ease_reg, default=OPTIONAL_FLAGS["ease_reg"])
    p.add_argument("--ease_neighbours", type=ease_neighbours, default=OPTIONAL_FLAGS["ease_neighbours"])
    p.add_argument("--liked_min_rating", type=cli.unit_float, default=OPTIONAL_FLAGS["liked_min_rating"])
    return p


def query_of(args):
    """("anime", name | None for a random one) or ("user", id): ValueError unless exactly one query is named."""
    anime = str(args.anime_query).strip()
    has_anime = bool(args.random_anime) or anime.lower() not in ("", "none")
    has_user = args.user_query != "none"
    if has_anime == has_user:
        raise ValueError("ease_recs takes exactly one of --anime_query (or --random_anime) and --user_query (got %s)"
                         % ("both" if has_anime else "neither"))
    return ("user", int(args.user_query)) if has_user else ("anime", None if args.random_anime else anime)


def go(args):
    import pandas as pd
    kind, query = query_of(args)
    main_df = pd.read_parquet(artifacts.use_artifact(args.main_df, args.main_df_type))
    anime_df = C.load_anime_df(artifacts.use_artifact(args.anime_df, args.anime_df_type))
    syn_df = C.load_synopses(artifacts.use_artifact(args.sypnopses_df, args.sypnopsis_df_type))
    types = C.literal(args.types) if args.spec_types else None
    genres = C.literal(args.anime_rec_genres) if args.an_spec_genres else None
    fit_args = (args.liked_min_rating, args.ease_reg, args.ease_neighbours)
    meta = {"Main data frame used": args.main_df}
    if kind == "anime":
        if query is None:
            rated = anime_df[anime_df.anime_id.isin(main_df.anime_id.unique())]
            query = random.choice(rated["Name"].dropna().unique().tolist())
            logger.info("Using %s as random input anime", query)
        frame, fn, stats = C.ease_similar_frame(main_df, anime_df, syn_df, query, int(args.a_query_number), types, genres,
                                                *fit_args)
        what = "Anime with the largest EASE weights from: " + str(query)
        meta.update({"Queried anime": query})
    else:
        frame, stats = C.ease_recs_frame(main_df, anime_df, syn_df, query, int(args.a_query_number), types, genres,
                                         *fit_args)
        fn = "User_ID_%d_ease_recs.csv" % query
        what = "EASE recommendations for user %d" % query
        meta.update({"Queried user": query})
    frame.to_csv(fn, index=False)
    artifacts.log_artifact(fn, fn, args.a_rec_type, what, metadata=dict(meta, Filename=fn, **stats))
    if not args.save_sim_anime:
        os.remove(fn)
    return frame


if __name__ == "__main__":
    cli.run("ease_recs", logger, go, make_parser())
