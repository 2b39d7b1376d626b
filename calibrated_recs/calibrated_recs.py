#!/usr/bin/env python
"""calibrated_recs component — model_recs with the list calibrated to the user's own taste profile.  The reference ranks
a user's unwatched anime by predicted rating alone (model_recs.py:373-456) and shows the user's favourite profile only
as word clouds (user_prefs.py:95-136); a rating head amplifies the majority taste, so favourites that are 70 % action
and 30 % romance give a top-10 that is all action.  Here the ``--pool`` best candidates (same user selection, same Type
/ Genre filters: the model_recs flag set as it is) are re-ranked greedily (``recs.calibrated_topk``): each pick
maximises ``(1 - calibration) * rating - calibration * (the total variation distance between the Genres (or Source)
token proportions of the list so far and those of the user's favourites)``.  ``--calibration 0`` is model_recs' own
list.  Writes ``User_ID_<id>_calibrated_<model_recs_fn>``: the model_recs columns plus ``Miscalibration``; the
artifact's metadata carries calibration, pool, the column, the user's number of favourites and the miscalibration of
the list and of the plain top-k."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import cli, components as C  # noqa: E402
from anime_recommendations_amd.cli import (MODEL_RECS_BOOL_FLAGS as BOOL_FLAGS,  # noqa: E402
                                           MODEL_RECS_STR_FLAGS as STR_FLAGS, select_user)

OPTIONAL_FLAGS = {"calibration": 0.5, "pool": 100, "calibration_column": "Genres", "favorite_percentile": 80.0}

logger = C.setup_logging("calibrated_recs")


def make_parser():
    p = C.make_parser("Get anime recommendations calibrated to the user's favourite profile", STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--calibration", type=cli.unit_float, default=OPTIONAL_FLAGS["calibration"])
    p.add_argument("--pool", type=int, default=OPTIONAL_FLAGS["pool"])
    p.add_argument("--calibration_column", choices=C.CALIBRATION_COLUMNS, default=OPTIONAL_FLAGS["calibration_column"])
    p.add_argument("--favorite_percentile", type=cli.percentile, default=OPTIONAL_FLAGS["favorite_percentile"])
    return p


def go(args):
    inp = cli.load_inputs(args)
    user = select_user(args, inp.df)
    logger.info("Using %s as input user; calibration %s on %s, pool %d", user, args.calibration,
                args.calibration_column, args.pool)
    frame, stats = C.calibrated_recs_frame(*inp.tables, user, int(args.model_num_recs), **cli.filters(args),
                                           pool=args.pool, calibration=args.calibration,
                                           column=args.calibration_column,
                                           favorite_percentile=args.favorite_percentile)
    fn = "User_ID_" + str(user) + "_calibrated_" + args.model_recs_fn
    return cli.write_recs(args, frame, fn, "calibrated_" + args.model_recs_fn,
                          "Calibrated anime recs based on model rankings for user : " + str(user),
                          {"Queried user: ": user, "Filename": fn, **stats})


if __name__ == "__main__":
    cli.run("calibrated_recs", logger, go, make_parser())
