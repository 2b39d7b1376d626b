#!/usr/bin/env python
"""new_user_recs component — model_recs for users the model was NOT trained on.  The reference reads the user's row
out of the trained table (model_recs.py:373-394) and so serves training users only; here every user of a ratings file
(``user_id, anime_id, rating``: the preprocess output schema, rating in [0, 1]) gets a row fitted to their own ratings
with the rest of the model frozen (``recs.fold_in_users``), and the queried user's unwatched anime are ranked with it.
Writes ``User_ID_<id>_<model_recs_fn>`` for the queried user (``--user_query``, else the first user of the file),
``folded_users.npz`` (ids, rows, loss of every user of the file) and, with ``--fold_neighbours true``,
``User_<id>.csv``: the trained users closest to the folded row.  The model_recs flags that pick a TRAINED user
(``model_user_query``, ``model_ID_conf``, ``model_ID_flow``, ``flow_ID``, ``flow_ID_type``, ``random_user``) are
accepted, so that a model_recs flag set can be passed on as it is, and not read: such a user is not in the file."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, cli, components as C  # noqa: E402

STR_FLAGS = cli.MODEL_RECS_STR_FLAGS + ["new_ratings", "fold_steps", "fold_lr"]
BOOL_FLAGS = cli.MODEL_RECS_BOOL_FLAGS + ["fold_neighbours"]
OPTIONAL_FLAGS = ["user_query"]     # "None" or absent: see select_user
FOLDED_FN = "folded_users.npz"
NEIGHBOURS, NUM_FAVES = 10, 3       # the reference's similar_users defaults (id_query_number, num_faves)

logger = C.setup_logging("new_user_recs")


def make_parser():
    p = C.make_parser("Recommend anime to users the model was not trained on", STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--user_query", type=str, default="None")
    return p


def read_ratings(path):
    import pandas as pd
    return pd.read_csv(path) if str(path).lower().endswith(".csv") else pd.read_parquet(path)


def select_user(args, new_df):
    if str(args.user_query) not in ("None", ""):
        return int(args.user_query)
    return int(new_df["user_id"].iloc[0])


def go(args):
    import numpy as np
    inp = cli.load_inputs(args, main_df=False)
    new_df = read_ratings(artifacts.use_artifact(args.new_ratings))
    user = select_user(args, new_df)
    logger.info("Using %s as input user; %d new users in %s", user, new_df["user_id"].nunique(), args.new_ratings)
    frame, folded = C.new_user_recs_frame(inp.model, new_df, inp.anime_df, inp.syn_df, user, int(args.model_num_recs),
                                          **cli.filters(args), steps=int(args.fold_steps), lr=float(args.fold_lr))
    if folded["n_dropped"]:
        logger.info("%d ratings of anime the model has no row for were dropped", folded["n_dropped"])
    np.savez(FOLDED_FN, ids=folded["ids"], rows=folded["rows"].cpu().numpy(), loss=folded["loss"].cpu().numpy())
    artifacts.log_artifact(FOLDED_FN, FOLDED_FN, "npz", "Folded-in rows of the users of " + str(args.new_ratings),
                           metadata={"n_users": int(len(folded["ids"])), "fold_steps": int(args.fold_steps),
                                     "fold_lr": float(args.fold_lr), "n_dropped": folded["n_dropped"]})
    fn = "User_ID_" + str(user) + "_" + args.model_recs_fn
    cli.write_recs(args, frame, fn, args.model_recs_fn, "Anime recs based on model rankings for new user : " + str(user),
                   {"Queried user: ": user, "Filename": fn})
    if args.fold_neighbours:
        near, nfn = C.new_user_neighbours_frame(inp.model, folded, cli.main_frame(args), inp.anime_df, user, NEIGHBOURS,
                                                NUM_FAVES, False)
        near.to_csv(nfn, index=False)
    return frame


if __name__ == "__main__":
    cli.run("new_user_recs", logger, go, make_parser())
