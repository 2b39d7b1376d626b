#!/usr/bin/env python
"""user_prefs component — drop-in for user_prefs/user_prefs.py of the reference: a user's favourite anime
(ratings at or above --favorite_percentile of the user's own ratings) and word clouds of their Genres and Source
tokens; writes ``User_ID_<id>_<prefs_csv>`` and the two cloud PNGs as artefacts."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, cli, components as C  # noqa: E402

STR_FLAGS = ["model", "main_df", "project_name", "anime_df", "prefs_user_query", "favorite_percentile", "genre_fn",
             "source_fn", "cloud_width", "cloud_height", "prefs_csv", "interval", "flow_user", "main_df_type",
             "anime_df_type", "ID_type", "cloud_type", "fave_art_type"]
BOOL_FLAGS = ["show_clouds", "save_faves", "prefs_from_flow", "prefs_local_user"]

logger = C.setup_logging("user_prefs")


def select_user(args, df):
    """select_user (user_prefs.py:292-323): the MLflow ID artefact, the config user, or a random user."""
    import pandas as pd
    if args.prefs_from_flow:
        user = int(pd.read_csv(artifacts.use_artifact(args.flow_user, args.ID_type)).values[0][0])
        logger.info("Using %s as input use taken from MLflow", user)
        return user, "MLflow ID"
    if args.prefs_local_user:
        user = int(args.prefs_user_query)
        logger.info("Using %s as config file-specified input user", user)
        return user, "Local Config File ID"
    user = C.random_user(df)
    logger.info("Using %s as random input user", user)
    return user, "Random User"


def go(args):
    import pandas as pd
    from anime_recommendations_amd import weights_io
    df = pd.read_parquet(artifacts.use_artifact(args.main_df, args.main_df_type))
    anime_df = C.load_user_anime_df(artifacts.use_artifact(args.anime_df, args.anime_df_type))
    model = weights_io.load_model(artifacts.use_artifact(args.model))
    user_ids, anime_ids = C.index_tables(model, df)
    user, user_type = select_user(args, df)
    fav = C.favourite_bits(df, user_ids, anime_ids, float(args.favorite_percentile))
    fave_df, genre_freq, source_freq = C.user_prefs_frame(fav, user_ids, anime_ids, anime_df, user)

    genre_fn = "User_ID_" + str(user) + "_" + args.genre_fn
    source_fn = "User_ID_" + str(user) + "_" + args.source_fn
    fave_fn = "User_ID_" + str(user) + "_" + args.prefs_csv
    genres_cloud = C.word_cloud(genre_freq, genre_fn, args.cloud_width, args.cloud_height, "white", "spring")
    sources_cloud = C.word_cloud(source_freq, source_fn, args.cloud_width, args.cloud_height, "gray", "autumn")
    fave_df.to_csv(fave_fn)

    artifacts.log_artifact(args.genre_fn, genre_fn, args.cloud_type, "Cloud image of favorite genres",
                           metadata={"ID": user, "User_type": user_type, "Filename": genre_fn})
    artifacts.log_artifact(args.source_fn, source_fn, args.cloud_type, "Image of source cloud",
                           metadata={"ID": user, "User_Type": user_type, "Filename": source_fn})
    artifacts.log_artifact(args.prefs_csv, fave_fn, args.fave_art_type,
                           "Csv file of a users favorite Genres and sources",
                           metadata={"ID": user, "User_Type": user_type, "Filename": fave_fn})
    logger.info("Favorites data frame logged!")
    if args.show_clouds:
        C.show_cloud(genres_cloud, args.interval)
        C.show_cloud(sources_cloud, args.interval)
    if not args.save_faves:
        os.remove(genre_fn)
        os.remove(source_fn)
        os.remove(fave_fn)
    return fave_df, genre_freq, source_freq


if __name__ == "__main__":
    cli.run("user_prefs", logger, go, C.make_parser("Get user preferences", STR_FLAGS, BOOL_FLAGS))
