#!/usr/bin/env python
"""explain_recs component — model_recs with a reason beside every row.  The reference lists what the model predicts
(model_recs.py:373-456) and cannot say why; the model can: a predicted rating sees an anime only through the cosine of
its row with the user's, so a listed anime is explained by the anime of the user's OWN ratings whose rows lie closest
to it, each weighted by what the user gave it (``recs.explain_topk``).  The model_recs flag set as it is, plus

    --explain_count <1..8>                  reasons per listed anime (default 3)
    --explain_weight rating|similarity      rating * cosine (default), or the cosine alone
    --explain_min_rating <float in [0, 1]>  only the user's ratings at or above it count as reasons (default 0.0)

Writes ``User_ID_<id>_explained_<model_recs_fn>``: the model_recs columns with the same values, then per reason
``Because_r``, ``Because_r_rating``, ``Because_r_similarity``, ``Because_r_contribution`` (empty where there is no
reason with a contribution above 0); the artifact's metadata carries the three values."""
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
OPTIONAL_FLAGS = {"explain_count": 3, "explain_weight": "rating", "explain_min_rating": 0.0}

logger = C.setup_logging("explain_recs")


def explain_count(v):
    try:
        n = int(str(v).strip())
    except ValueError:
        n = None
    if n is None or not 1 <= n <= C.EXPLAIN_MAX_COUNT:
        raise ValueError("%r is not an integer in 1 .. %d" % (v, C.EXPLAIN_MAX_COUNT))
    return n


def explain_weight(v):
    s = str(v).strip().lower()
    if s not in C.EXPLAIN_WEIGHTS:
        raise ValueError("%r is not one of %s" % (v, ", ".join(C.EXPLAIN_WEIGHTS)))
    return s


def explain_min_rating(v):
    try:
        x = float(v)
    except (TypeError, ValueError):
        x = float("nan")
    if not 0.0 <= x <= 1.0:             # (a NaN fails both comparisons)
        raise ValueError("%r is not a number in [0, 1]" % (v,))
    return x


def make_parser():
    p = C.make_parser("Get anime recommendations from the ranking model, each with the user's ratings behind it",
                      STR_FLAGS, BOOL_FLAGS)
    p.add_argument("--explain_count", type=explain_count, default=OPTIONAL_FLAGS["explain_count"])
    p.add_argument("--explain_weight", type=explain_weight, default=OPTIONAL_FLAGS["explain_weight"])
    p.add_argument("--explain_min_rating", type=explain_min_rating, default=OPTIONAL_FLAGS["explain_min_rating"])
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
    logger.info("Using %s as input user; %d reasons by %s, ratings from %s", user, args.explain_count,
                args.explain_weight, args.explain_min_rating)
    frame = C.explain_recs_frame(model["U"], model["A"], weights_io.model_head(model), user_ids, anime_ids, df,
                                 anime_df, syn_df, user, int(args.model_num_recs),
                                 types=C.literal(args.anime_types) if args.specify_types else None,
                                 genres=C.literal(args.model_genres) if args.specify_genres else None,
                                 count=args.explain_count, weight=args.explain_weight,
                                 min_rating=args.explain_min_rating)
    fn = "User_ID_" + str(user) + "_explained_" + args.model_recs_fn
    frame.to_csv(fn, index=False)
    artifacts.log_artifact("explained_" + args.model_recs_fn, fn, args.model_recs_type,
                           "Anime recs based on model rankings, with the ratings behind them, for user : " + str(user),
                           metadata={"Queried user: ": user, "Filename": fn, "explain_count": args.explain_count,
                                     "explain_weight": args.explain_weight,
                                     "explain_min_rating": args.explain_min_rating})
    if not args.save_model_recs:
        os.remove(fn)
    return frame


if __name__ == "__main__":
    _args = make_parser().parse_args()
    try:
        go(_args)
    except Exception:                      # non-zero exit + the reason in ./explain_recs.log
        logger.exception("explain_recs failed")
        raise
