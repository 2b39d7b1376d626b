#!/usr/bin/env python
"""user_recs component — drop-in for user_recs/user_recs.py of the reference: anime recommended to a user by how
many of its most similar users hold them as favourites (80th percentile of their own ratings), the user's own
favourites skipped; writes ``User_ID_<id>_<user_recs_fn>``, ``User_ID_<id>_<ID_recs_faves_fn>`` and the two
``User_ID_<id>_recs_favorite_*.png`` word clouds as artefacts."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, cli, components as C  # noqa: E402

STR_FLAGS = ["main_df", "project_name", "anime_df", "user_recs_query", "user_recs_fn", "sypnopses_df",
             "user_num_recs", "model", "ID_emb_name", "anime_emb_name", "main_df_type", "anime_df_type",
             "sypnopsis_df_type", "model_type", "user_recs_type", "flow_ID", "flow_ID_type", "sim_users_art",
             "sim_users_art_type", "recs_n_sim_ID", "ID_rec_genres", "prefs_input_fn", "prefs_input_type",
             "ID_recs_faves_fn", "ID_recs_faves_type", "n_flow_sim_IDs"]
BOOL_FLAGS = ["save_user_recs", "recs_ID_from_conf", "ID_spec_genres", "ID_recs_from_flow", "raise_flow_error"]
PERCENTILE = 80.0        # user_recs.py:348-388 fave_genres / fave_sources: np.percentile(watched.rating, 80)

logger = C.setup_logging("user_recs")


def flow_id(args):
    import pandas as pd
    return int(pd.read_csv(artifacts.use_artifact(args.flow_ID, args.flow_ID_type)).values[0][0])


def select_user(args, df):
    """select_user (user_recs.py:530-556): the MLflow ID artefact, the config user, or a random user."""
    if args.ID_recs_from_flow:
        user = flow_id(args)
        logger.info("Using %s as input from MLflow in select_user()", user)
    elif args.recs_ID_from_conf:
        user = int(args.user_recs_query)
        logger.info("Using %s as config specified in select_user()", user)
    else:
        user = C.random_user(df)
        logger.info("Using %s as random input user in select_user()", user)
    return user


def assert_flow(args, user):
    """assert_flow (user_recs.py:632-679): the queried user of the ID, similar-users and prefs artefacts agree, and
    the similar-users artefact holds --recs_n_sim_ID users."""
    id_art = flow_id(args)
    sim_meta = artifacts.artifact_metadata(args.sim_users_art)
    prefs_meta = artifacts.artifact_metadata(args.prefs_input_fn)
    sim_id, n_sim, prefs_id = int(sim_meta["Queried user"]), int(sim_meta["num_sim_users"]), int(prefs_meta["ID"])
    if user == id_art == sim_id == prefs_id and n_sim == int(args.recs_n_sim_ID):
        logger.info("ID %s is consistent in assert_flow(), using MLflow", user)
        return True
    logger.info("MLflow failed assert_flow()! IDs were inconsistent!")
    logger.info("Input ID was %s, ID artifact was %s, similar users ID was %s, user prefs ID was %s", user, id_art,
                sim_id, prefs_id)
    logger.info("Num sim users in artifact was %s, input num sim users was %s", n_sim, int(args.recs_n_sim_ID))
    return False


def go(args):
    import numpy as np
    import pandas as pd
    import torch
    from anime_recommendations_amd import ops, weights_io
    C.check_user_recs_limits(int(args.recs_n_sim_ID), int(args.user_num_recs))
    df = pd.read_parquet(artifacts.use_artifact(args.main_df, args.main_df_type))
    anime_df = C.load_user_anime_df(artifacts.use_artifact(args.anime_df, args.anime_df_type))
    syn_df = C.load_synopses(artifacts.use_artifact(args.sypnopses_df, args.sypnopsis_df_type))
    model = weights_io.load_model(artifacts.use_artifact(args.model, args.model_type), args.ID_emb_name,
                                  args.anime_emb_name)
    user_ids, anime_ids = C.index_tables(model, df)
    user = select_user(args, df)
    fav = C.favourite_bits(df, user_ids, anime_ids, PERCENTILE)

    if args.ID_recs_from_flow:
        sim_df = pd.read_csv(artifacts.use_artifact(args.sim_users_art, args.sim_users_art_type))
        sim_ids = sim_df["similar_users"].to_numpy()
        logger.info("Using sim users artifact, sim users are %s", sim_ids)
        fave_df = pd.read_csv(artifacts.use_artifact(args.prefs_input_fn, args.prefs_input_type))
        if not assert_flow(args, user):
            if args.raise_flow_error:
                raise ValueError("MLflow IDs were inconsistent")
            logger.info("MLflow IDs were inconsistent. Process terminated.")
            return None
        C.check_user_recs_limits(len(sim_ids), int(args.user_num_recs))
        meta = C.metadata_by_index(anime_ids, anime_df)
        genre_freq, source_freq = C.favourite_profiles(fav, meta, [C.user_index(user_ids, user)])[0]
    else:
        u = C.user_index(user_ids, user)
        Uh = ops.rownorm(torch.as_tensor(model["U"]))
        idx, _ = ops.cosine_topk(Uh, [u], int(args.recs_n_sim_ID), exclude_self=True)
        idx = idx.cpu().numpy()[0]
        sim_ids = np.asarray(user_ids)[idx[idx >= 0]]
        fave_df, genre_freq, source_freq = C.user_prefs_frame(fav, user_ids, anime_ids, anime_df, user)

    genres = C.literal(args.ID_rec_genres) if args.ID_spec_genres else None
    recs_df = C.user_recs_frame(fav, user_ids, anime_ids, anime_df, syn_df, sim_ids, fave_df,
                                int(args.user_num_recs), genres)
    filename = "User_ID_" + str(user) + "_" + args.user_recs_fn
    recs_df.to_csv(filename, index=False)
    genre_fn = "User_ID_" + str(user) + "_recs_favorite_genres.png"
    source_fn = "User_ID_" + str(user) + "_recs_favorite_sources.png"
    C.word_cloud(genre_freq, genre_fn, 600, 350, "white", "spring")
    C.word_cloud(source_freq, source_fn, 600, 350, "gray", "autumn")
    fave_fn = "User_ID_" + str(user) + "_" + args.ID_recs_faves_fn
    fave_df.to_csv(fave_fn, index=False)

    artifacts.log_artifact(args.user_recs_fn, filename, args.user_recs_type,
                           "Anime recs based on user prefs: " + str(user),
                           metadata={"Queried user": user, "Flow ID used": args.ID_recs_from_flow,
                                     "Filename": filename})
    artifacts.log_artifact(genre_fn, genre_fn, "png", "Cloud image of favorite genres",
                           metadata={"Queried user": user, "Filename": genre_fn})
    artifacts.log_artifact(source_fn, source_fn, "png", "Image of source cloud",
                           metadata={"Queried user": user, "Filename": source_fn})
    artifacts.log_artifact(args.ID_recs_faves_fn, fave_fn, args.ID_recs_faves_type,
                           "Csv file of a users favorite Genres and sources",
                           metadata={"Queried user": user, "Filename": fave_fn})
    logger.info("Favorites data frame logged!")
    if not args.save_user_recs:
        for f in (filename, source_fn, fave_fn, genre_fn):
            os.remove(f)
    return recs_df


if __name__ == "__main__":
    cli.run("user_recs", logger, go, C.make_parser("Get user preferences", STR_FLAGS, BOOL_FLAGS))
