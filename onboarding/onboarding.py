#!/usr/bin/env python
"""onboarding component — which anime to show a newcomer so that there is something to fit: a greedy maximum-coverage
questionnaire from the rating frame alone.  No model takes part.  also_liked's data and filter flags without the query
flags, ``--onboard_fn`` (the CSV's name), ``--onboard_type`` (the artifact type), ``--save_onboard``, plus

    --onboard_number <int 1..1024>          how many anime the list holds (default 20)
    --onboard_depth <int >= 1>              a user counts as served once it has rated this many of the list (default 3)
    --onboard_strategy coverage|popularity  greedy maximum coverage, or the most rated anime (default coverage)
    --onboard_max_ratings <int >= 0>        the population: users with at most this many ratings; 0 = everyone (default 0)
    --onboard_holdout <0 <= float < 1>      the share of the population that takes no part in the picking (default 0.2)
    --onboard_seed <int >= 0>               the seed of the split (default 0)

The CSV holds similar_anime's metadata columns, ``Rated_by``, ``New_reach`` and ``Reach_share``.  The artifact's metadata
holds the figures of BOTH strategies on the same split — on the pick users and on the held-out users, the share knowing
at least one listed anime, the share knowing ``onboard_depth`` of them, the mean number known.  The picks run in
libanirec (HIP): AND + popcount of every rated-by bit row against the users still open, per pick."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, cli, components as C  # noqa: E402

STR_FLAGS = ["main_df_type", "anime_df_type", "sypnopsis_df_type", "project_name", "main_df", "sypnopses_df", "anime_df",
             "anime_rec_genres", "types", "onboard_fn", "onboard_type"]
BOOL_FLAGS = ["an_spec_genres", "spec_types", "save_onboard"]
OPTIONAL_FLAGS = {"onboard_number": 20, "onboard_depth": 3, "onboard_strategy": "coverage", "onboard_max_ratings": 0,
                  "onboard_holdout": 0.2, "onboard_seed": 0}
MAX_NUMBER = 1024

logger = C.setup_logging("onboarding")


def _refuse(v, allowed):
    """argparse prints an ArgumentTypeError's message (a ValueError's is dropped), so the error names what is allowed"""
    return argparse.ArgumentTypeError("%r is not %s" % (v, allowed))


def _int(v, lo, hi, allowed):
    try:
        n = int(str(v).strip())
    except ValueError:
        n = None
    if n is None or not lo <= n <= hi:
        raise _refuse(v, allowed)
    return n


def onboard_number(v):
    return _int(v, 1, MAX_NUMBER, "an integer in 1 .. %d" % MAX_NUMBER)


def onboard_depth(v):
    return _int(v, 1, 2 ** 31 - 1, "an integer >= 1")


def onboard_strategy(v):
    s = str(v).strip().lower()
    if s not in C.ONBOARD_STRATEGIES:
        raise _refuse(v, "one of " + ", ".join(C.ONBOARD_STRATEGIES))
    return s


def onboard_max_ratings(v):
    return _int(v, 0, 2 ** 31 - 1, "an integer >= 0 (0 = every user)")


def onboard_holdout(v):
    try:
        x = float(str(v).strip())
    except ValueError:
        x = -1.0
    if not 0.0 <= x < 1.0:
        raise _refuse(v, "a share in 0 <= x < 1")
    return x


def onboard_seed(v):
    return _int(v, 0, 2 ** 63 - 1, "an integer >= 0")


def make_parser():
    p = C.make_parser("Anime to ask a newcomer about: a greedy maximum-coverage list", STR_FLAGS, BOOL_FLAGS)
    for f, default in OPTIONAL_FLAGS.items():
        p.add_argument("--" + f, type=globals()[f], default=default)
    return p


def go(args):
    import pandas as pd
    anime_df = C.load_anime_df(artifacts.use_artifact(args.anime_df, args.anime_df_type))
    syn_df = C.load_synopses(artifacts.use_artifact(args.sypnopses_df, args.sypnopsis_df_type))
    main_df = pd.read_parquet(artifacts.use_artifact(args.main_df, args.main_df_type))
    frame, summary = C.onboarding_frame(
        main_df, anime_df, syn_df, args.onboard_number, args.onboard_depth, args.onboard_strategy,
        types=C.literal(args.types) if args.spec_types else None,
        genres=C.literal(args.anime_rec_genres) if args.an_spec_genres else None,
        max_ratings=args.onboard_max_ratings, holdout=args.onboard_holdout, seed=args.onboard_seed)
    logger.info("onboarding summary: %s", json.dumps(summary, sort_keys=True))
    fn = args.onboard_fn
    frame.to_csv(fn, index=False)
    artifacts.log_artifact(fn, fn, args.onboard_type, "Anime to ask a newcomer about (%s)" % args.onboard_strategy,
                           metadata=dict(summary, **{"Main data frame used": args.main_df, "Filename": fn}))
    if not args.save_onboard:
        os.remove(fn)
    return frame


if __name__ == "__main__":
    cli.run("onboarding", logger, go, make_parser())
