#!/usr/bin/env python
"""rp3_recs component — lists from RP3beta (Paudel et al. 2017; P3alpha, Cooper et al. 2014), the three-step random walk
over the liked pairs with a popularity penalty: the anime with the largest weights in a query anime's row, or one user's
list among the anime they have not rated.  No neural model takes part; the fit is a user-weighted co-occurrence on the
i8 matrix cores.  also_liked's data and filter flags, plus

    --user_query <user id | none>    list for this user instead of an anime (default none)
    --rp3_alpha <float >= 0>         the exponent of the user and start-item degrees (default 1: the plain walk)
    --rp3_beta <float >= 0>          the popularity penalty on the end item (default 0.3; 0 = P3alpha)
    --rp3_neighbours <K>             the largest weights every anime keeps (default 100; 0 = the dense matrix)
    --liked_min_rating <0..1>        the scaled rating from which a rating counts as liked (default 0.0)

The defaults are common values from the literature; none is tuned on this data.  Exactly one of --anime_query and
--user_query (or --random_anime) names the query.  With an anime the CSV holds similar_anime's columns (``Similarity`` is
the weight W[query, anime]); with a user, model_recs' columns with ``Rp3_score`` in the place of the predicted rating.
The weighted sums, the score rows and the select run in libanirec (HIP): DESIGN.md §4.25."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, cli, components as C  # noqa: E402

STR_FLAGS = ["main_df_type", "anime_df_type", "sypnopsis_df_type", "project_name", "main_df", "sypnopses_df", "anime_df",
             "anime_query", "a_query_number", "anime_rec_genres", "types", "a_rec_type"]
BOOL_FLAGS = ["random_anime", "an_spec_genres", "spec_types", "save_sim_anime"]
OPTIONAL_FLAGS = {"user_query": "none", "rp3_alpha": cli.RP3_FLAGS["rp3_alpha"][1],
                  "rp3_beta": cli.RP3_FLAGS["rp3_beta"][1], "rp3_neighbours": cli.RP3_FLAGS["rp3_neighbours"][1],
                  "liked_min_rating": 0.0}

logger = C.setup_logging("rp3_recs")


def user_query(v):
    s = str(v).strip()
    return "none" if s.lower() in ("", "none") else str(int(s))


def rp3_exponent(v):
    x = float(str(v).strip())
    if not 0.0 <= x < float("inf"):
        raise ValueError("%r is not a finite exponent >= 0" % (v,))
    return x


def rp3_neighbours(v):
    k = int(str(v).strip())
    if k < 0:
        raise ValueError("%r is not a count >= 0" % (v,))
    return k


def make_parser():
    p = C.make_parser("Lists from the RP3beta random-walk model of the liked pairs", STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--user_query", type=user_query, default=OPTIONAL_FLAGS["user_query"])
    p.add_argument("--rp3_alpha", type=rp3_exponent, default=OPTIONAL_FLAGS["rp3_alpha"])
    p.add_argument("--rp3_beta", type=rp3_exponent, default=OPTIONAL_FLAGS["rp3_beta"])
    p.add_argument("--rp3_neighbours", type=rp3_neighbours, default=OPTIONAL_FLAGS["rp3_neighbours"])
    p.add_argument("--liked_min_rating", type=cli.unit_float, default=OPTIONAL_FLAGS["liked_min_rating"])
    return p


def query_of(args):
    """("anime", name | None for a random one) or ("user", id): ValueError unless exactly one query is named."""
    anime = str(args.anime_query).strip()
    has_anime = bool(args.random_anime) or anime.lower() not in ("", "none")
    has_user = args.user_query != "none"
    if has_anime == has_user:
        raise ValueError("rp3_recs takes exactly one of --anime_query (or --random_anime) and --user_query (got %s)"
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
    fit_args = (args.liked_min_rating, args.rp3_alpha, args.rp3_beta, args.rp3_neighbours)
    meta = {"Main data frame used": args.main_df}
    if kind == "anime":
        if query is None:
            rated = anime_df[anime_df.anime_id.isin(main_df.anime_id.unique())]
            query = random.choice(rated["Name"].dropna().unique().tolist())
            logger.info("Using %s as random input anime", query)
        frame, fn, stats = C.rp3_similar_frame(main_df, anime_df, syn_df, query, int(args.a_query_number), types, genres,
                                               *fit_args)
        what = "Anime with the largest RP3beta weights from: " + str(query)
        meta.update({"Queried anime": query})
    else:
        frame, stats = C.rp3_recs_frame(main_df, anime_df, syn_df, query, int(args.a_query_number), types, genres,
                                        *fit_args)
        fn = "User_ID_%d_rp3_recs.csv" % query
        what = "RP3beta recommendations for user %d" % query
        meta.update({"Queried user": query})
    frame.to_csv(fn, index=False)
    artifacts.log_artifact(fn, fn, args.a_rec_type, what, metadata=dict(meta, Filename=fn, **stats))
    if not args.save_sim_anime:
        os.remove(fn)
    return frame


if __name__ == "__main__":
    cli.run("rp3_recs", logger, go, make_parser())
