"""Command-line plumbing the component scripts share.  ``run`` is every script's ``__main__`` tail; the rest serves the
model_recs family (model_recs, diverse_recs, calibrated_recs, explain_recs, group_recs, new_user_recs, hybrid_recs), whose
scripts
answer one question with one flag set: its flags, the user pick, the input artifacts, the Type / Genre filters and the
CSV-and-artifact a run leaves behind.  A script of the family keeps what is its own: its extra flags, its log line, its
``components.*_frame`` call, its file and artifact names and its metadata."""
from __future__ import annotations

import os
import random
from typing import NamedTuple

from . import artifacts, components as C

# the reference's model_recs flags, all required (tests/golden/component_flags.json)
MODEL_RECS_STR_FLAGS = ["main_df", "main_df_type", "project_name", "anime_df", "anime_df_type", "sypnopsis_df",
                        "sypnopsis_df_type", "model", "model_type", "model_user_query", "model_recs_fn", "model_num_recs",
                        "anime_types", "model_genres", "model_recs_type", "flow_ID", "flow_ID_type"]
MODEL_RECS_BOOL_FLAGS = ["random_user", "save_model_recs", "specify_types", "specify_genres", "model_ID_flow",
                         "model_ID_conf"]


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


# the flags of a hybrid list (hybrid_recs; evaluate --baseline hybrid): all optional.  Equal weights and rrf_c = 60 are the
# literature's defaults, not tuned on this data.
HYBRID_FLAGS = {
    "hybrid_systems": (str, "model,itemknn,als", "the systems whose score rows are fused, separated by a comma: model, "
                                                 "popularity, itemknn, als, content, ease, rp3, bpr"),
    "hybrid_weights": (str, "none", "none (all 1), or a list with one weight >= 0 per system, e.g. \"[1, 1, 0.5]\""),
    "hybrid_method": (str, "rrf", "rrf (reciprocal rank fusion) or minmax (the sum of min-max normalised scores)"),
    "hybrid_rrf_c": (int, 60, "the constant of reciprocal rank fusion: a term is weight / (rrf_c + rank), rank from 1"),
}


# the flags of an EASE fit (ease_recs; evaluate --baseline ease): all optional.  reg = 500 is the paper's value (Steck
# 2019) for a data set of about this many users, not tuned on this data.
EASE_FLAGS = {
    "ease_reg": (float, 500.0, "the L2 weight of the EASE fit, > 0: the larger, the more the weights shrink"),
    "ease_neighbours": (int, 0, "K > 0 keeps the K largest weights of every anime only; 0 = the dense model"),
}


# the flags of an RP3beta fit (rp3_recs; evaluate --baseline rp3): all optional.  alpha = 1, beta = 0.3 and 100
# neighbours are common values from the literature (Paudel et al. 2017), not tuned on this data.
RP3_FLAGS = {
    "rp3_alpha": (float, 1.0, "the exponent of the user and start-item degrees, >= 0: 1 is the plain random walk"),
    "rp3_beta": (float, 0.3, "the popularity penalty on the end item, >= 0: 0 is P3alpha"),
    "rp3_neighbours": (int, 100, "the largest weights every anime keeps; 0 = the dense matrix"),
}


def hybrid_args(args):
    """The ``systems`` / ``weights`` / ``method`` / ``rrf_c`` of the HYBRID_FLAGS on ``args`` (the defaults where a parser
    has none of them)."""
    def get(f):
        return getattr(args, f, HYBRID_FLAGS[f][1])
    weights = str(get("hybrid_weights")).strip()
    return {"systems": tuple(x.strip().lower() for x in str(get("hybrid_systems")).split(",") if x.strip()),
            "weights": None if weights.lower() == "none" else list(C.literal(weights)),
            "method": str(get("hybrid_method")).strip().lower(), "rrf_c": int(get("hybrid_rrf_c"))}


def add_flags(parser, flags):
    for flag, (kind, default, text) in flags.items():
        parser.add_argument("--" + flag, type=kind, default=default, required=False, help=text)
    return parser


def select_user(args, df):
    """select_user (model_recs.py:334-370): the user of the MLflow run (flow_ID artifact), the configured one, or a
    random one."""
    import pandas as pd
    if args.model_ID_flow:
        flow = pd.read_csv(artifacts.use_artifact(args.flow_ID, args.flow_ID_type))
        return int(flow["User_ID"].values[0])
    if args.model_ID_conf:
        return int(args.model_user_query)
    return int(random.choice(df["user_id"].unique().tolist()))


class Inputs(NamedTuple):
    """What a run reads.  ``tables`` is the leading (U, A, head, user_ids, anime_ids, df, anime_df, syn_df) of every
    ``components.*_recs_frame`` signature; it and ``df`` are None when the main frame was not asked for."""
    model: dict
    df: object
    anime_df: object
    syn_df: object
    tables: tuple


def main_frame(args):
    import pandas as pd
    return pd.read_parquet(artifacts.use_artifact(args.main_df, args.main_df_type))


def load_inputs(args, main_df=True):
    """The input artifacts of a model_recs flag set.  ``main_df`` False skips the rating frame and, with it, the index
    tables (new_user_recs, whose users are not in it)."""
    from . import weights_io
    df = main_frame(args) if main_df else None
    anime_df = C.load_anime_df(artifacts.use_artifact(args.anime_df, args.anime_df_type))
    syn_df = C.load_synopses(artifacts.use_artifact(args.sypnopsis_df, args.sypnopsis_df_type))
    model = weights_io.load_model(artifacts.use_artifact(args.model, args.model_type))
    if not main_df:
        return Inputs(model, None, anime_df, syn_df, None)
    user_ids, anime_ids = C.index_tables(model, df)
    return Inputs(model, df, anime_df, syn_df,
                  (model["U"], model["A"], weights_io.model_head(model), user_ids, anime_ids, df, anime_df, syn_df))


def filters(args):
    """The ``types=`` / ``genres=`` pair of a ``*_frame`` call: a filter is None unless its ``specify_*`` flag is set."""
    return {"types": C.literal(args.anime_types) if args.specify_types else None,
            "genres": C.literal(args.model_genres) if args.specify_genres else None}


def write_recs(args, frame, fn, name, description, metadata):
    """Write ``frame`` to ``fn``, log it as artifact ``name`` (type ``model_recs_type``) and remove the local file
    unless ``save_model_recs``.  Returns ``frame``."""
    frame.to_csv(fn, index=False)
    artifacts.log_artifact(name, fn, args.model_recs_type, description, metadata=metadata)
    if not args.save_model_recs:
        os.remove(fn)
    return frame


def run(name, logger, go, parser):
    """A component script's ``__main__``: parse, run, and on failure exit non-zero with the reason in ``./<name>.log``
    (SURVEY §8(b))."""
    args = parser.parse_args()
    try:
        go(args)
    except Exception:
        logger.exception("%s failed", name)
        raise
