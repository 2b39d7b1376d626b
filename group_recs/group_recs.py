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
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import cli, components as C  # noqa: E402
from anime_recommendations_amd.cli import (MODEL_RECS_BOOL_FLAGS as BOOL_FLAGS,  # noqa: E402
                                           MODEL_RECS_STR_FLAGS as STR_FLAGS, select_user)

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


def go(args):
    inp = cli.load_inputs(args)
    members = list(args.group_users) or [select_user(args, inp.df)]
    logger.info("Using %s as the group; strategy %s, floor %s", members, args.group_strategy, args.group_floor)
    frame = C.group_recs_frame(*inp.tables, members, int(args.model_num_recs), **cli.filters(args),
                               strategy=args.group_strategy, floor=args.group_floor)
    fn = "Group_" + C.group_label(members) + "_" + args.model_recs_fn
    return cli.write_recs(args, frame, fn, "group_" + args.model_recs_fn,
                          "Anime recs based on model rankings for the group : " + str(members),
                          {"Group members: ": members, "Filename": fn, "strategy": args.group_strategy,
                           "floor": args.group_floor})


if __name__ == "__main__":
    cli.run("group_recs", logger, go, make_parser())
