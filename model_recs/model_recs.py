#!/usr/bin/env python
"""model_recs component — drop-in for model_recs/model_recs.py of the reference: rank every
anime a user has not watched by the model's predicted rating (``model.predict``), optional
Type / Genre filters, top ``model_num_recs`` to ``User_ID_<id>_<model_recs_fn>``."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import cli, components as C  # noqa: E402
from anime_recommendations_amd.cli import (MODEL_RECS_BOOL_FLAGS as BOOL_FLAGS,  # noqa: E402
                                           MODEL_RECS_STR_FLAGS as STR_FLAGS, select_user)

logger = C.setup_logging("model_recs")


def go(args):
    inp = cli.load_inputs(args)
    user = select_user(args, inp.df)
    logger.info("Using %s as input user", user)
    frame = C.model_recs_frame(*inp.tables, user, int(args.model_num_recs), **cli.filters(args))
    fn = "User_ID_" + str(user) + "_" + args.model_recs_fn
    return cli.write_recs(args, frame, fn, args.model_recs_fn,
                          "Anime recs based on model rankings for user : " + str(user),
                          {"Queried user: ": user, "Filename": fn})


if __name__ == "__main__":
    cli.run("model_recs", logger, go,
            C.make_parser("Get anime recommendations from the ranking model", STR_FLAGS, BOOL_FLAGS))
