#!/usr/bin/env python
"""diverse_recs component — model_recs with the list diversified.  The reference ranks a user's unwatched anime by
predicted rating alone (model_recs.py:373-456), and the rating sees an anime only through the cosine of its embedding
row with the user's: the seasons, specials and movies of one franchise, whose rows nearly coincide, enter a top-10
together.  Here the ``--pool`` best candidates (same user selection, same Type / Genre filters: the model_recs flag
set as it is) are re-ranked greedily (maximal marginal relevance, ``recs.diverse_topk``): each pick maximises
``(1 - diversity) * rating - diversity * (largest cosine to an anime already picked)``.  ``--diversity 0`` is
model_recs' own list.  Writes ``User_ID_<id>_diverse_<model_recs_fn>``: the model_recs columns plus
``Max_similarity``; the artifact's metadata carries diversity, pool and the mean pairwise cosine of the list and of
the plain top-k."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import cli, components as C  # noqa: E402
from anime_recommendations_amd.cli import (MODEL_RECS_BOOL_FLAGS as BOOL_FLAGS,  # noqa: E402
                                           MODEL_RECS_STR_FLAGS as STR_FLAGS, select_user)

OPTIONAL_FLAGS = {"diversity": 0.3, "pool": 100}

logger = C.setup_logging("diverse_recs")


def make_parser():
    p = C.make_parser("Get diversified anime recommendations from the ranking model", STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--diversity", type=cli.unit_float, default=OPTIONAL_FLAGS["diversity"])
    p.add_argument("--pool", type=int, default=OPTIONAL_FLAGS["pool"])
    return p


def go(args):
    inp = cli.load_inputs(args)
    user = select_user(args, inp.df)
    logger.info("Using %s as input user; diversity %s, pool %d", user, args.diversity, args.pool)
    frame, stats = C.diverse_recs_frame(*inp.tables, user, int(args.model_num_recs), **cli.filters(args),
                                        pool=args.pool, diversity=args.diversity)
    fn = "User_ID_" + str(user) + "_diverse_" + args.model_recs_fn
    return cli.write_recs(args, frame, fn, "diverse_" + args.model_recs_fn,
                          "Diversified anime recs based on model rankings for user : " + str(user),
                          {"Queried user: ": user, "Filename": fn, "diversity": args.diversity, "pool": args.pool,
                           **stats})


if __name__ == "__main__":
    cli.run("diverse_recs", logger, go, make_parser())
