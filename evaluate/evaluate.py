#!/usr/bin/env python
"""evaluate component — how well a trained model RANKS: the ratings the neural_network run held out for validation
(the last ``test_size`` rows of the same encoding and RandomState(42) shuffle) are ranked among the anime their user
has no training rating for, by predicted rating, and hit rate / NDCG at each ``eval_k``, MRR and the mean and median
rank are written to ``eval_csv``; ``--baseline popularity`` adds the same figures for ranking by rating count alone, to
read the model's against, ``--baseline itemknn`` those of an item-kNN over co-occurrence counts fitted on the training
slice alone, ``--baseline als`` those of an implicit-feedback ALS factorisation fitted on the same slice (a comma list
gives several; the ``--itemknn_*`` and ``--als_*`` flags of the command line set their parameters, which are the usual
library defaults and have not been tuned on this data), ``--baseline hybrid`` those of the fused score rows of several
systems (``--hybrid_systems model,itemknn,als``, ``--hybrid_method rrf|minmax``, ``--hybrid_weights``, ``--hybrid_rrf_c``:
command line only; equal weights and rrf_c = 60 are the literature's defaults, not tuned on this data either),
``--baseline hybrid_tuned`` those of the same fusion with weights chosen from a grid, every user's targets ranked with
the weights that scored best on the OTHER folds of users (``--hybrid_tune_metric``, ``--hybrid_tune_steps``,
``--hybrid_tune_folds``, ``--hybrid_tune_seed``: command line only), ``--baseline content`` those of the content-based
system over all_anime.csv's columns (``--anime_df``, ``--sypnopses_df``, ``--content_columns``, ``--content_weight``,
``--content_min_rating``: command line only; also a member ``--hybrid_systems`` takes), ``--baseline ease`` those of
EASE, the closed-form linear item-item model fitted on the training slice (``--ease_reg``, ``--ease_min_rating``,
``--ease_neighbours``: command line only; reg = 500 is the paper's value for a data set of about this many users, not
tuned on this data; also a member ``--hybrid_systems`` takes), ``--baseline rp3`` those of RP3beta, the three-step random
walk with a popularity penalty fitted on the training slice (``--rp3_alpha``, ``--rp3_beta``, ``--rp3_neighbours``,
``--rp3_min_rating``: command line only; 1, 0.3 and 100 are common values from the literature, not tuned on this data; also
a member ``--hybrid_systems`` takes), ``--baseline bpr`` those of a BPR matrix factorisation, the learned model with a
pairwise objective, fitted on the training slice (``--bpr_factors``, ``--bpr_epochs``, ``--bpr_batch``, ``--bpr_lr``,
``--bpr_reg``, ``--bpr_tries``, ``--bpr_bias``, ``--bpr_min_rating``, ``--bpr_seed``: command line only; the literature's and
the ``implicit`` library's common values, not tuned on this data; also a member ``--hybrid_systems`` takes);
``--lists_diversity "[0, 0.3]"`` adds ``lists_csv``: what each diverse_recs diversity costs in hits and buys in
spread, over every held-out user's top ``lists_k`` list; ``--ci_replicates 1000`` adds a bootstrap interval over the
held-out users to every figure and a paired difference and p-value against every other system, ``--compare_model`` a
second model as one of those systems (command line only, like the ``--itemknn_*`` flags).  The reference has no such step:
its author lists comparing re-trained models as an idea for improvement; ``val_loss`` cannot compare models across
losses and activations, these figures can."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from anime_recommendations_amd import artifacts, cli, components as C  # noqa: E402

STR_FLAGS = ["input_data", "main_df_type", "model", "model_type", "project_name", "test_size", "eval_k", "min_rating",
             "eval_csv", "eval_type", "ID_emb_name", "anime_emb_name"]
BOOL_FLAGS = []
# optional: the accuracy / diversity trade-off of the model's top-k lists (components.evaluate_lists_frame)
OPTIONAL_FLAGS = {
    "lists_diversity": (str, "none", "none, or a list of diverse_recs --diversity values, e.g. \"[0, 0.1, 0.3, 0.5]\": "
                                     "hit rate and spread of every held-out user's top list at each value"),
    "lists_k": (int, 10, "the length of those lists"),
    "lists_pool": (int, 100, "the candidates the re-rank picks from (diverse_recs --pool)"),
    "lists_csv": (str, "eval_lists.csv", "the file the list figures are written to, logged as an eval_type artifact"),
}

# optional and command-line only (not MLproject parameters; `mlflow run` takes the defaults): the item-kNN baseline
ITEMKNN_FLAGS = {
    "itemknn_neighbours": (int, 50, "neighbours every anime keeps"),
    "itemknn_measure": (str, "cosine", "cosine, jaccard or confidence of the liked-by sets"),
    "itemknn_shrink": (float, 0.0, "added to the measure's denominator"),
    "itemknn_min_support": (int, 1, "users two anime must share to be neighbours"),
    "itemknn_min_rating": (float, 0.0, "the scaled rating (0..1) from which a training rating counts as liked"),
}

# optional and command-line only, like the item-kNN flags: the implicit-feedback ALS baseline (components.ALS_DEFAULTS:
# the usual library defaults with the width moved to the nearest supported one, not tuned on this data)
ALS_FLAGS = {
    "als_factors": (int, 64, "the width of the factor tables: 32, 64, 128 or 256"),
    "als_sweeps": (int, 15, "sweeps, each a user half and an item half"),
    "als_cg_steps": (int, 3, "conjugate-gradient steps per row and half-sweep (0 .. 16)"),
    "als_alpha": (float, 1.0, "a liked pair's confidence is 1 + alpha"),
    "als_reg": (float, 0.01, "the L2 weight on both factor tables"),
    "als_min_rating": (float, 0.0, "the scaled rating (0..1) from which a training rating counts as liked"),
    "als_seed": (int, 0, "the seed of the start tables"),
}

# optional and command-line only, like the item-kNN flags: confidence intervals and a second model to compare with
CI_FLAGS = {
    "ci_replicates": (int, 0, "bootstrap replicates over the held-out users (0: no intervals): every figure gains a "
                              "percentile interval, every other system a paired difference and a p-value"),
    "ci_level": (float, 0.95, "the level of those intervals"),
    "ci_seed": (int, 0, "the seed of the bootstrap weights"),
    "compare_model": (str, "none", "none, or a second model artifact (of model_type, over the same id tables): ranked on "
                                   "the same targets and reported as the system compare"),
}

# optional and command-line only, like the item-kNN flags: the members and the fusion of --baseline hybrid
# (components.HYBRID_DEFAULTS: equal weights and rrf_c = 60, the literature's defaults, not tuned on this data)
HYBRID_FLAGS = cli.HYBRID_FLAGS

# optional and command-line only: how --baseline hybrid_tuned chooses its weights (components.HYBRID_TUNE_DEFAULTS)
HYBRID_TUNE_FLAGS = {
    "hybrid_tune_metric": (str, "ndcg@10", "the figure the weights are chosen by: ndcg@K, hit_rate@K or mrr"),
    "hybrid_tune_steps": (int, 10, "the grid: equal weights and every weight vector of multiples of 1 / steps with sum 1"),
    "hybrid_tune_folds": (int, 2, "folds of held-out users (>= 2): a user's targets are ranked with the weights that "
                                  "scored best on the other folds"),
    "hybrid_tune_seed": (int, 0, "the seed of the deal of users into folds"),
}

# optional and command-line only, like the item-kNN flags: the content-based system (--baseline content, or a member of
# --hybrid_systems; components.CONTENT_DEFAULTS).  It scores from all_anime.csv, so it needs --anime_df
CONTENT_FLAGS = {
    "anime_df": (str, "none", "none, or the all_anime.csv artifact: the metadata the content system scores from"),
    "anime_df_type": (str, "raw_data", "the type of that artifact"),
    "sypnopses_df": (str, "none", "none, or the synopsis artifact (for --content_columns with Sypnopsis)"),
    "sypnopsis_df_type": (str, "raw_data", "the type of that artifact"),
    "content_columns": (str, ",".join(C.CONTENT_DEFAULTS["columns"]), "the columns the item vectors are built from, "
                                                                      "separated by a comma (Sypnopsis is opt-in)"),
    "content_weight": (str, C.CONTENT_DEFAULTS["weight"], "rating, centered or one: how a training rating weighs its "
                                                          "title in the user's profile"),
    "content_min_rating": (float, C.CONTENT_DEFAULTS["min_rating"], "the scaled rating (0..1) from which a training "
                                                                    "rating enters the profile"),
}

# optional and command-line only, like the item-kNN flags: EASE (--baseline ease, or a member of --hybrid_systems;
# components.EASE_DEFAULTS: reg = 500 is the paper's value for a data set of about this many users, not tuned on this data)
EASE_FLAGS = dict(cli.EASE_FLAGS, ease_min_rating=(float, C.EASE_DEFAULTS["min_rating"],
                                                   "the scaled rating (0..1) from which a training rating counts as liked"))

# optional and command-line only, like the item-kNN flags: RP3beta (--baseline rp3, or a member of --hybrid_systems;
# components.RP3_DEFAULTS: common values from the literature, not tuned on this data)
RP3_FLAGS = dict(cli.RP3_FLAGS, rp3_min_rating=(float, C.RP3_DEFAULTS["min_rating"],
                                                "the scaled rating (0..1) from which a training rating counts as liked"))

# optional and command-line only, like the item-kNN flags: BPR matrix factorisation (--baseline bpr, or a member of
# --hybrid_systems; components.BPR_DEFAULTS: the literature's and the ``implicit`` library's common values with the width
# moved to the nearest supported one, not tuned on this data)
BPR_FLAGS = {
    "bpr_factors": (int, C.BPR_DEFAULTS["factors"], "the width of the factor tables: 32, 64, 128 or 256"),
    "bpr_epochs": (int, C.BPR_DEFAULTS["epochs"], "epochs, each ceil(liked pairs / batch) steps"),
    "bpr_batch": (int, C.BPR_DEFAULTS["batch"], "sampled triples per step"),
    "bpr_lr": (float, C.BPR_DEFAULTS["lr"], "the learning rate"),
    "bpr_reg": (float, C.BPR_DEFAULTS["reg"], "the L2 weight on both factor tables"),
    "bpr_tries": (int, C.BPR_DEFAULTS["tries"], "negative candidates drawn per triple before it is dropped (1 .. 16)"),
    "bpr_bias": (C.str2bool, C.BPR_DEFAULTS["bias"], "whether the last factor column is an item bias"),
    "bpr_min_rating": (float, C.BPR_DEFAULTS["min_rating"],
                       "the scaled rating (0..1) from which a training rating counts as liked"),
    "bpr_seed": (int, C.BPR_DEFAULTS["seed"], "the seed of the start tables and the sampler"),
}

logger = C.setup_logging("evaluate")


def baseline_arg(text):
    """``--baseline``: none, a name, or a comma list of names -> evaluate_frame's ``baseline`` (None, or a list)."""
    names = [b.strip().lower() for b in str(text).split(",") if b.strip()]
    if not names or names == ["none"]:
        return None
    return names


def _content_flag(args, f):
    return getattr(args, f, CONTENT_FLAGS[f][1])


def wants(args, system):
    """whether ``system`` takes part: as a baseline, or as a member of a hybrid that is asked for"""
    names = baseline_arg(args.baseline) or []
    fused = {"hybrid", "hybrid_tuned"} & set(names)
    return system in names or bool(fused and system in cli.hybrid_args(args)["systems"])


def wants_content(args):
    """whether the content system takes part"""
    return wants(args, "content")


def content_args(args, anime_ids=None):
    """evaluate_frame's ``content``: the content flags and, with ``anime_ids``, the metadata by that index.  ValueError
    without --anime_df."""
    if str(_content_flag(args, "anime_df")).lower() == "none":
        raise ValueError("--baseline content (and content as a hybrid member) scores from the anime metadata: give "
                         "--anime_df (command line only)")
    par = {"columns": [c.strip() for c in str(_content_flag(args, "content_columns")).split(",") if c.strip()],
           "weight": _content_flag(args, "content_weight"), "min_rating": float(_content_flag(args, "content_min_rating")),
           "meta": ()}
    if anime_ids is not None:
        anime_df = C.load_anime_df(artifacts.use_artifact(args.anime_df, _content_flag(args, "anime_df_type")))
        syn = str(_content_flag(args, "sypnopses_df"))
        syn_df = None if syn.lower() == "none" else \
            C.load_synopses(artifacts.use_artifact(syn, _content_flag(args, "sypnopsis_df_type")))
        par["meta"] = C.metadata_by_index(anime_ids, anime_df, syn_df)
    return par


def ease_args(args):
    """evaluate_frame's ``ease``: the EASE flags the parser has"""
    return {f[len("ease_"):]: getattr(args, f) for f in EASE_FLAGS if hasattr(args, f)}


def rp3_args(args):
    """evaluate_frame's ``rp3``: the RP3 flags the parser has"""
    return {f[len("rp3_"):]: getattr(args, f) for f in RP3_FLAGS if hasattr(args, f)}


def bpr_args(args):
    """evaluate_frame's ``bpr``: the BPR flags the parser has"""
    return {f[len("bpr_"):]: getattr(args, f) for f in BPR_FLAGS if hasattr(args, f)}


def go(args):
    content = None
    if wants(args, "bpr"):                                  # the cheap failures: before any file or GPU use
        C._system_params({"bpr": bpr_args(args)}, ["bpr"])
    if wants(args, "rp3"):                                  # the cheap failures: before any file or GPU use
        C._system_params({"rp3": rp3_args(args)}, ["rp3"])
    if wants(args, "ease"):                                 # the cheap failures: before any file or GPU use
        C._system_params({"ease": ease_args(args)}, ["ease"])
    if wants_content(args):                                 # the cheap failures: before any file or GPU use
        C._system_params({"content": content_args(args)}, ["content"])
    from anime_recommendations_amd import weights_io
    model = weights_io.load_model(artifacts.use_artifact(args.model, args.model_type), args.ID_emb_name,
                                  args.anime_emb_name)
    from anime_recommendations_amd import ingest            # (torch: after the cheap failures)
    table = ingest.load_user_stats(artifacts.use_artifact(args.input_data, args.main_df_type))
    logger.info("Final df shape is (%d, 3); %d users, %d anime", len(table), table.n_users, table.n_anime)
    ci = {f: getattr(args, f, CI_FLAGS[f][1]) for f in ("ci_replicates", "ci_level", "ci_seed")}
    compare = str(getattr(args, "compare_model", "none"))
    if wants_content(args):
        content = content_args(args, table.anime_ids)
    compare_model = None
    if compare.lower() != "none":
        compare_model = weights_io.load_model(artifacts.use_artifact(compare, args.model_type), args.ID_emb_name,
                                              args.anime_emb_name)
    frame, summary = C.evaluate_frame(model, table, int(args.test_size), C.literal(args.eval_k),
                                      float(args.min_rating), baseline=baseline_arg(args.baseline),
                                      itemknn={f[len("itemknn_"):]: getattr(args, f) for f in ITEMKNN_FLAGS
                                               if hasattr(args, f)},
                                      als={f[len("als_"):]: getattr(args, f) for f in ALS_FLAGS if hasattr(args, f)},
                                      compare_model=compare_model, hybrid=cli.hybrid_args(args),
                                      hybrid_tune={f[len("hybrid_tune_"):]: getattr(args, f) for f in HYBRID_TUNE_FLAGS
                                                   if hasattr(args, f)}, content=content, ease=ease_args(args),
                                      rp3=rp3_args(args), bpr=bpr_args(args), **ci)
    frame.to_csv(args.eval_csv, index=False)
    artifacts.log_artifact(args.eval_csv, args.eval_csv, args.eval_type,
                           "Ranking metrics of the held-out ratings for model : " + str(args.model),
                           metadata={k: v for k, v in summary.items()})
    logger.info("Ranking metrics: %s", summary)
    if args.lists_diversity.lower() != "none":
        lists, lists_summary = C.evaluate_lists_frame(model, table, int(args.test_size), float(args.min_rating),
                                                      C.literal(args.lists_diversity), int(args.lists_k),
                                                      int(args.lists_pool), **ci)
        lists.to_csv(args.lists_csv, index=False)
        artifacts.log_artifact(args.lists_csv, args.lists_csv, args.eval_type,
                               "Hits and spread of the top-%d lists per diversity for model : %s"
                               % (int(args.lists_k), args.model), metadata=dict(lists_summary))
        logger.info("List metrics: %s", lists_summary)
        summary = dict(summary, **lists_summary)
    print(json.dumps(summary))
    return frame, summary


def make_parser():
    parser = C.make_parser("Rank the held-out ratings with a trained model", STR_FLAGS, BOOL_FLAGS)
    # optional, unlike the flags above: "popularity" adds the figures of recommending the most-rated unseen anime
    parser.add_argument("--baseline", type=str, default="none", required=False,
                        help="none, popularity (rank the same targets by the anime's number of training ratings), "
                             "itemknn (by an item-kNN over co-occurrence counts of the training ratings), als (by an "
                             "implicit-feedback ALS factorisation of the training ratings), hybrid (by the fused "
                             "score rows of several of them and the model), hybrid_tuned (the same with cross-fitted "
                             "weights from a grid), content (by TF-IDF vectors of the anime metadata; needs "
                             "--anime_df), ease (by the closed-form linear item-item model EASE fitted on the "
                             "training ratings), rp3 (by the RP3beta random walk over the training ratings), bpr "
                             "(by a BPR matrix factorisation fitted on the training ratings), or several separated "
                             "by a comma")
    for flag, (kind, default, text) in OPTIONAL_FLAGS.items():
        parser.add_argument("--" + flag, type=kind, default=default, required=False, help=text)
    return parser


def make_cli_parser():
    """``make_parser`` (the MLproject's parameters) and the command-line-only ``--itemknn_*``, ``--als_*``, ``--ci_*``,
    ``--compare_model``, ``--hybrid_*``, ``--hybrid_tune_*``, content (``CONTENT_FLAGS``), ``--ease_*``, ``--rp3_*`` and
    ``--bpr_*`` flags."""
    parser = make_parser()
    for flag, (kind, default, text) in list(ITEMKNN_FLAGS.items()) + list(ALS_FLAGS.items()) + list(CI_FLAGS.items()) + \
            list(HYBRID_FLAGS.items()) + list(HYBRID_TUNE_FLAGS.items()) + list(CONTENT_FLAGS.items()) + \
            list(EASE_FLAGS.items()) + list(RP3_FLAGS.items()) + list(BPR_FLAGS.items()):
        parser.add_argument("--" + flag, type=kind, default=default, required=False, help=text)
    return parser


if __name__ == "__main__":
    cli.run("evaluate", logger, go, make_cli_parser())
