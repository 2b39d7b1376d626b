#!/usr/bin/env python
"""also_liked component — "people who liked this also liked ...": the anime most often liked together with a query
anime, from the rating frame alone.  No model takes part, so it serves before a neural_network run exists and gives a
trained one something to be read against.  similar_anime's flags and filters without the model flags, plus

    --liked_min_rating <0..1>            the scaled rating from which a rating counts as liked (default 0.0: every rating)
    --cooc_measure cosine|jaccard|confidence   how two liked-by sets are compared (default cosine)
    --cooc_shrink <float >= 0>           added to the measure's denominator: damps anime few users liked (default 0)
    --cooc_min_support <int >= 0>        users two anime must share to be listed together (default 1)

The CSV holds similar_anime's columns (``Similarity`` is the measure), ``Liked_by_both`` and ``Liked_by``.  The counts
run in libanirec (HIP): AND + popcount over the liked-by bit rows, then the exact select."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, cli, components as C  # noqa: E402

STR_FLAGS = ["main_df_type", "anime_df_type", "sypnopsis_df_type", "project_name", "main_df", "sypnopses_df", "anime_df",
             "anime_query", "a_query_number", "anime_rec_genres", "types", "a_rec_type"]
BOOL_FLAGS = ["random_anime", "an_spec_genres", "spec_types", "save_sim_anime"]
OPTIONAL_FLAGS = {"liked_min_rating": 0.0, "cooc_measure": "cosine", "cooc_shrink": 0.0, "cooc_min_support": 1}

logger = C.setup_logging("also_liked")


def liked_min_rating(v):
    x = float(str(v).strip())
    if not 0.0 <= x <= 1.0:
        raise ValueError("%r is not a scaled rating in 0 .. 1" % (v,))
    return x


def cooc_measure(v):
    s = str(v).strip().lower()
    if s not in C.COOC_MEASURES:
        raise ValueError("%r is not one of %s" % (v, ", ".join(C.COOC_MEASURES)))
    return s


def cooc_shrink(v):
    x = float(str(v).strip())
    if not 0.0 <= x < float("inf"):
        raise ValueError("%r is not a finite number >= 0" % (v,))
    return x


def cooc_min_support(v):
    n = int(str(v).strip())
    if n < 0:
        raise ValueError("%r is not an integer >= 0" % (v,))
    return n


def make_parser():
    p = C.make_parser("Anime most often liked together with a query anime", STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--liked_min_rating", type=liked_min_rating, default=OPTIONAL_FLAGS["liked_min_rating"])
    p.add_argument("--cooc_measure", type=cooc_measure, default=OPTIONAL_FLAGS["cooc_measure"])
    p.add_argument("--cooc_shrink", type=cooc_shrink, default=OPTIONAL_FLAGS["cooc_shrink"])
    p.add_argument("--cooc_min_support", type=cooc_min_support, default=OPTIONAL_FLAGS["cooc_min_support"])
    return p


def go(args):
    import pandas as pd
    anime_df = C.load_anime_df(artifacts.use_artifact(args.anime_df, args.anime_df_type))
    syn_df = C.load_synopses(artifacts.use_artifact(args.sypnopses_df, args.sypnopsis_df_type))
    main_df = pd.read_parquet(artifacts.use_artifact(args.main_df, args.main_df_type))
    if args.random_anime:
        name = random.choice(anime_df["Name"].dropna().unique().tolist())
        logger.info("Using %s as random input anime", name)
    else:
        name = args.anime_query
    frame, fn = C.also_liked_frame(
        main_df, anime_df, syn_df, name, int(args.a_query_number),
        types=C.literal(args.types) if args.spec_types else None,
        genres=C.literal(args.anime_rec_genres) if args.an_spec_genres else None,
        liked_min_rating=args.liked_min_rating, measure=args.cooc_measure, shrink=args.cooc_shrink,
        min_support=args.cooc_min_support)
    frame.to_csv(fn, index=False)
    artifacts.log_artifact(fn, fn, args.a_rec_type, "Anime liked together with: " + str(name),
                           metadata={"Queried anime": name, "Main data frame used": args.main_df, "Filename": fn,
                                     "liked_min_rating": args.liked_min_rating, "cooc_measure": args.cooc_measure,
                                     "cooc_shrink": args.cooc_shrink, "cooc_min_support": args.cooc_min_support})
    if not args.save_sim_anime:
        os.remove(fn)
    return frame


if __name__ == "__main__":
    cli.run("also_liked", logger, go, make_parser())
