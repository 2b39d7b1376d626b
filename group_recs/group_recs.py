#!/usr/bin/env python
"""group_recs component — model_recs for several users who watch together.  The reference answers for one user at a
time (model_recs.py:373-456); a group's list is not the intersection of its members' lists, and the rating
``act(hs * cos(u, a) + hb)`` of a mean embedding row is not the mean of the ratings.  Here the members' exact ratings
(the bits of model_recs) are aggregated per anime and ranked among the anime NO member has rated (``ops.group_topk``),
under the same Type / Genre filters: the model_recs flag set as it is, plus

    --group_users "[id, id, ...]"   the members; empty or absent: the selected user alone, which is model_recs' list
    --group_strategy                mean | least_misery (the lowest member rating) | most_pleasure (the highest)
    --group_floor <float>           optional: an anime any member rates below it is no candidate

Writes ``Group_<ids joined by _>_<model_recs_fn>`` (above 8 members ``Group_<first id>_and_<n-1>_more_...``): the
model_recs columns with ``Prediction`` the aggregate, ``Min_prediction``, ``Max_prediction`` and one ``User_<id>``
column per member; the artifact's metadata carries the members, the strategy and the floor."""
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
OPTIONAL_FLAGS = {"group_users": "[]", "group_strategy": "mean", "group_floor": None}

logger = C.setup_logging("group_recs")


def strategy(v):
    s = str(v).strip().lower()
    if s not in C.GROUP_STRATEGIES:
        raise ValueError("%r is not one of %s" % (v, ", ".join(C.GROUP_STRATEGIES)))
    return s


def optional_float(v):
    """a float, or None for an empty value / ``none``; NaN is refused"""
    if v is None or str(v).strip().lower() in ("", "none"):
        return None
    x = float(v)
    if x != x:
        raise ValueError("the floor is NaN")
    return x


def user_list(v):
    """``"[id, id, ...]"`` (or an empty value) as a list of ints"""
    try:
        ids = C.literal(v) if isinstance(v, str) and v.strip() else []
        return [int(u) for u in ([ids] if isinstance(ids, int) else ids)]
    except (SyntaxError, TypeError) as e:
        raise ValueError("%r is not a list of user ids" % (v,)) from e


def make_parser():
    p = C.make_parser("Get anime recommendations for a group of users from the ranking model", STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--group_users", type=user_list, default=[])
    p.add_argument("--group_strategy", type=strategy, default=OPTIONAL_FLAGS["group_strategy"])
    p.add_argument("--group_floor", type=optional_float, default=OPTIONAL_FLAGS["group_floor"])
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
    members = list(args.group_users) or [select_user(args, df)]
    logger.info("Using %s as the group; strategy %s, floor %s", members, args.group_strategy, args.group_floor)
    frame = C.group_recs_frame(model["U"], model["A"], weights_io.model_head(model), user_ids, anime_ids, df, anime_df,
                               syn_df, members, int(args.model_num_recs),
                               types=C.literal(args.anime_types) if args.specify_types else None,
                               genres=C.literal(args.model_genres) if args.specify_genres else None,
                               strategy=args.group_strategy, floor=args.group_floor)
    fn = "Group_" + C.group_label(members) + "_" + args.model_recs_fn
    frame.to_csv(fn, index=False)
    artifacts.log_artifact("group_" + args.model_recs_fn, fn, args.model_recs_type,
                           "Anime recs based on model rankings for the group : " + str(members),
                           metadata={"Group members: ": members, "Filename": fn, "strategy": args.group_strategy,
                                     "floor": args.group_floor})
    if not args.save_model_recs:
        os.remove(fn)
    return frame


if __name__ == "__main__":
    _args = make_parser().parse_args()
    try:
        go(_args)
    except Exception:                      # non-zero exit + the reason in ./group_recs.log
        logger.exception("group_recs failed")
        raise
