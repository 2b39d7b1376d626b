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
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, components as C  # noqa: E402

# the model_recs flag set, as it is
STR_FLAGS = ["main_df", "main_df_type", "project_name", "anime_df", "anime_df_type", "sypnopsis_df",
             "sypnopsis_df_type", "model", "model_type", "model_user_query", "model_recs_fn", "model_num_recs",
             "anime_types", "model_genres", "model_recs_type", "flow_ID", "flow_ID_type"]
BOOL_FLAGS = ["random_user", "save_model_recs", "specify_types", "specify_genres", "model_ID_flow", "model_ID_conf"]
OPTIONAL_FLAGS = {"calibration": 0.5, "pool": 100, "calibration_column": "Genres", "favorite_percentile": 80.0}

logger = C.setup_logging("calibrated_recs")


def unit_float(v):
    x = float(v)
    if not 0.0 <= x <= 1.0:
        raise ValueError("%r is not in [0, 1]" % (v,))
    return x


def percentile(v):
    x = float(v)
    if not 0.0 <= x <= 100.0:
        raise ValueError("%r is not in [0, 100]" % (v,))
    return x


def make_parser():
    p = C.make_parser("Get anime recommendations calibrated to the user's favourite profile", STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--calibration", type=unit_float, default=OPTIONAL_FLAGS["calibration"])
    p.add_argument("--pool", type=int, default=OPTIONAL_FLAGS["pool"])
    p.add_argument("--calibration_column", choices=C.CALIBRATION_COLUMNS, default=OPTIONAL_FLAGS["calibration_column"])
    p.add_argument("--favorite_percentile", type=percentile, default=OPTIONAL_FLAGS["favorite_percentile"])
    return p


def select_user(args, df):
    """select_user (model_recs.py:334-370), as the model_recs component has it: the user of the MLflow run (flow_ID
    artifact), the configured one, or a random one."""
    import pandas as pd
    if args.model_ID_flow:
        flow = pd.read_csv(artifacts.use_artifact(args.flow_ID, args.flow_ID_type))
        return int(flow["User_ID"].values[0])
    if args.model_ID_conf:
        return int(args.model_user_query)
    return int(random.choice(df["user_id"].unique().tolist()))


def go(args):
    import pandas as pd
    from anime_recommendations_amd import weights_io
    df = pd.read_parquet(artifacts.use_artifact(args.main_df, args.main_df_type))
    anime_df = C.load_anime_df(artifacts.use_artifact(args.anime_df, args.anime_df_type))
    syn_df = C.load_synopses(artifacts.use_artifact(args.sypnopsis_df, args.sypnopsis_df_type))
    model = weights_io.load_model(artifacts.use_artifact(args.model, args.model_type))
    user_ids, anime_ids = C.index_tables(model, df)
    user = select_user(args, df)
    logger.info("Using %s as input user; calibration %s on %s, pool %d", user, args.calibration,
                args.calibration_column, args.pool)
    frame, stats = C.calibrated_recs_frame(model["U"], model["A"], weights_io.model_head(model), user_ids, anime_ids, df,
                                           anime_df, syn_df, user, int(args.model_num_recs),
                                           types=C.literal(args.anime_types) if args.specify_types else None,
                                           genres=C.literal(args.model_genres) if args.specify_genres else None,
                                           pool=args.pool, calibration=args.calibration,
                                           column=args.calibration_column,
                                           favorite_percentile=args.favorite_percentile)
    fn = "User_ID_" + str(user) + "_calibrated_" + args.model_recs_fn
    frame.to_csv(fn, index=False)
    artifacts.log_artifact("calibrated_" + args.model_recs_fn, fn, args.model_recs_type,
                           "Calibrated anime recs based on model rankings for user : " + str(user),
                           metadata={"Queried user: ": user, "Filename": fn, **stats})
    if not args.save_model_recs:
        os.remove(fn)
    return frame


if __name__ == "__main__":
    _args = make_parser().parse_args()
    try:
        go(_args)
    except Exception:                      # non-zero exit + the reason in ./calibrated_recs.log
        logger.exception("calibrated_recs failed")
        raise
