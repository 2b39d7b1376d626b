"""Shared host logic of the four drop-in components (neural_network, similar_anime,
similar_users, model_recs): flag parsing in the reference's style, metadata tables, filters
and the CSV frames they write.  The math (row-normalise, cosine top-k, predict) is libanirec.

Reference behaviour mirrored here (file:line in each function).  The per-row pandas loops of
the reference (similar_anime.py:413-455, model_recs.py:403-445) are replaced by boolean masks
evaluated BEFORE the GPU top-k, which yields the same rows: filter -> sort desc -> head(k).
"""
from __future__ import annotations

import argparse
import ast
import logging
import re
import string
import unicodedata

import numpy as np
import pandas as pd

ANIME_TYPES = ['TV', 'OVA', 'Movie', 'Special', 'ONA', 'Music']
_IRREGULAR = "★♥☆♡½ß²"


def str2bool(v):
    """distutils.util.strtobool semantics used by every ``type=lambda x: bool(strtobool(x))`` flag."""
    s = str(v).strip().lower()
    if s in ("y", "yes", "t", "true", "on", "1"):
        return True
    if s in ("n", "no", "f", "false", "off", "0"):
        return False
    raise argparse.ArgumentTypeError("invalid truth value %r" % (v,))


def make_parser(description, str_flags, bool_flags):
    """All flags required, strings unless listed as bool — as in the reference's argparse blocks
    (e.g. neural_network.py:298-555)."""
    p = argparse.ArgumentParser(description=description, fromfile_prefix_chars="@")
    for f in str_flags:
        p.add_argument("--" + f, type=str, required=True)
    for f in bool_flags:
        p.add_argument("--" + f, type=str2bool, required=True)
    return p


def setup_logging(name):
    logging.basicConfig(filename="./%s.log" % name, level=logging.INFO, filemode="a",
                        format="%(asctime)s-%(name)s - %(levelname)s - %(message)s",
                        datefmt="%d %b %Y %H:%M:%S %Z", force=True)
    return logging.getLogger()


def clean(item):
    """Filename/lookup normalisation of titles and genres (similar_anime.py:242-277): special
    symbols and whitespace removed, non-word characters dropped, accents stripped, lower-cased."""
    if isinstance(item, (list, tuple)):
        return [clean(x) for x in item]
    s = str(item)
    for ch in _IRREGULAR:
        s = s.replace(ch, " ")
    s = s.translate({ord(c): None for c in string.whitespace})
    s = re.sub(r"\W+", "", s)
    s = "".join(c for c in unicodedata.normalize("NFKD", s) if not unicodedata.combining(c))
    return s.lower()


def load_anime_df(path):
    """get_anime_df (similar_anime.py:63-93): 'Unknown' -> NaN, id/name columns, cleaned english
    name for lookups, sorted by Score descending."""
    df = pd.read_csv(path)
    df = df.replace("Unknown", np.nan)
    df["anime_id"] = df["MAL_ID"]
    df["japanese_name"] = df["Japanese name"]
    df["eng_version"] = [clean(x) for x in df["Name"]]
    df = df.sort_values(by=["Score"], ascending=False, kind="quicksort", na_position="last")
    keep = ["anime_id", "eng_version", "Score", "Genres", "Episodes", "Premiered", "Studios",
            "japanese_name", "Name", "Type", "Source", "Rating", "Members"]
    return df[[c for c in keep if c in df.columns]]


def load_synopses(path):
    return pd.read_csv(path)


def all_genres(anime_df):
    """get_genres (similar_anime.py:174-192): the text of the list of distinct Genres cells is split on
    whitespace, every token stripped of non-alphanumerics; the fragments of the three multi-word genres
    (and 'nan') are dropped and 'Slice of Life', 'Super Power', 'Martial Arts', 'None' appended — so, as in
    the reference, any OTHER multi-word genre ("Shounen Ai") is only known by its fragments."""
    cells = anime_df["Genres"].unique().tolist()
    tokens = sorted({re.sub(r"[\W_]", "", t) for t in str(cells).split()})
    fragments = {"Slice", "of", "Life", "Martial", "Arts", "Super", "Power", "nan"}
    return sorted(t for t in tokens + ["Slice of Life", "Super Power", "Martial Arts", "None"] if t not in fragments)


def genre_mask(genres_col, wanted):
    """by_genre (similar_anime.py:279-340): keep rows whose Genres contain ANY of the (three)
    wanted genres; 'None' entries ignored.  The wanted genres are clean()ed, the column text is only
    lower-cased with spaces removed (:307-317) — so, as in the reference, a genre whose name holds
    punctuation ("Sci-Fi" -> "scifi" vs "sci-fi") matches nothing
    (tests/golden/ref_fn/genres.json holds the reference function's own outputs)."""
    wanted = [w for w in clean(list(wanted)) if w != "none"]
    col = [str(g).lower().replace(" ", "") for g in genres_col]
    m = np.zeros(len(col), bool)
    for w in wanted:
        m |= np.array([w in c for c in col], dtype=bool)
    return m


def _topk_count(asked, what, rows):
    """The k of a component's top-k call.  The reference returns as many rows as asked for (Frame[:count]),
    which is at most the rows a query can return: `rows` (n_anime - 1 for similar_anime, n_users - 1 for
    similar_users, n_anime for model_recs).  The count is clamped to it, so a huge request allocates no more
    than a whole ranking; the top-k calls take any k (above MAX_TOPK the large-k kernels)."""
    k = int(asked)
    if k < 1:
        raise ValueError("%s must be >= 1 (got %d)" % (what, k))
    return max(1, min(k, int(rows)))


def check_genres(wanted, anime_df):
    valid = set(clean(all_genres(anime_df)))
    for g in clean(list(wanted)):
        if g not in valid:
            raise ValueError("An invalid genre was input (%r). Select genres from %s" % (g, sorted(valid)))


def check_types(types):
    for t in types:
        if t not in ANIME_TYPES:
            raise ValueError("An invalid type was input (%r). Select from %s" % (t, ANIME_TYPES))
    return list(types)


def literal(s):
    return ast.literal_eval(s) if isinstance(s, str) else s


# ----------------------------------------------------------------------------------------
# index <-> id tables
# ----------------------------------------------------------------------------------------
def index_tables(model, main_df=None, min_ratings=None):
    """index->id arrays for users and anime.  Taken from the model file when present (written by
    the neural_network component); otherwise rebuilt from the rating frame exactly like the
    reference does (order of first appearance, similar_users.py:42-54)."""
    from .data import encode_ids
    if model.get("user_ids") is not None and model.get("anime_ids") is not None:
        return np.asarray(model["user_ids"]), np.asarray(model["anime_ids"])
    if main_df is None:
        raise ValueError("model file has no id tables and no main data frame was given")
    df = main_df
    if min_ratings:
        n = df["user_id"].value_counts(dropna=True)
        df = df[df["user_id"].isin(n[n >= int(min_ratings)].index)]
    _, uids = encode_ids(df["user_id"].to_numpy())
    _, aids = encode_ids(df["anime_id"].to_numpy())
    return uids, aids


def metadata_by_index(anime_ids, anime_df, syn_df=None):
    """Metadata rows aligned with the anime index (row i describes anime_ids[i]); `has_meta`
    False where the anime is missing from all_anime.csv (the reference's lookups would raise)."""
    meta = anime_df.drop_duplicates("anime_id").set_index("anime_id")
    out = meta.reindex(anime_ids)
    out["has_meta"] = out["Name"].notna().to_numpy()
    out["anime_id"] = np.asarray(anime_ids)
    if syn_df is not None:
        # "None" where the anime has no synopsis row (the reference's IndexError branch); an empty synopsis cell
        # stays NaN, as get_sypnopsis returns it
        syn = syn_df.drop_duplicates("MAL_ID").set_index("MAL_ID")["sypnopsis"]
        text = syn.reindex(anime_ids).to_numpy(dtype=object)
        out["Sypnopsis"] = np.where(np.isin(np.asarray(anime_ids), syn.index.to_numpy()), text, "None")
    else:
        out["Sypnopsis"] = "None"
    return out.reset_index(drop=True)


def filter_mask(meta, anime_df, types=None, genres=None):
    """Rows of `meta` (metadata_by_index) a recommendation may list: the anime has an all_anime.csv row, and its Type
    / Genres pass the optional filters (similar_anime.py:431-455, model_recs.py:429-448)."""
    keep = meta["has_meta"].to_numpy().copy()
    if types is not None:
        keep &= meta["Type"].isin(check_types(types)).to_numpy()
    if genres is not None:
        check_genres(genres, anime_df)
        keep &= genre_mask(meta["Genres"], genres)
    return keep


def unwatched_mask(df, anime_ids, user_id):
    """get_unwatched (model_recs.py:132-156): indexed anime the user has not rated."""
    watched_ids = set(df[df.user_id == int(user_id)].anime_id.values.tolist())
    return ~np.isin(np.asarray(anime_ids), list(watched_ids))


# ----------------------------------------------------------------------------------------
# similar_anime
# ----------------------------------------------------------------------------------------
def find_anime_id(name, anime_df):
    """Resolve a query title like anime_recs (similar_anime.py:389-399), in its order: a Name equal to the
    cleaned query, else the exact Name, else the cleaned query against the cleaned english names."""
    key = clean(name)
    for hit in (anime_df[anime_df.Name == key], anime_df[anime_df.Name == name], anime_df[anime_df.eng_version == key]):
        if len(hit):
            return int(hit.anime_id.values[0])
    raise ValueError("anime %r not found in the anime data frame" % (name,))


def _similar_anime_rows(meta, idx, sim):
    """The frame anime_recs returns (similar_anime.py:364-471) for one query's top-k: ``idx`` anime indices (-1 padded) with
    their similarities ``sim``, metadata from ``meta`` (metadata_by_index)."""
    ok = idx >= 0
    rows = meta.iloc[idx[ok]]
    return pd.DataFrame({
        "Name": rows["Name"].to_numpy(), "Similarity": sim[ok], "Genres": rows["Genres"].to_numpy(),
        "Sypnopsis": rows["Sypnopsis"].to_numpy(), "Episodes": rows["Episodes"].to_numpy(),
        "Japanese name": rows["japanese_name"].to_numpy(), "Studios": rows["Studios"].to_numpy(),
        "Premiered": rows["Premiered"].to_numpy(), "Score": rows["Score"].to_numpy(),
        "Type": rows["Type"].to_numpy(), "Source": rows["Source"].to_numpy(),
        "Rating": rows["Rating"].to_numpy()})


def similar_anime_frame(A, anime_ids, anime_df, syn_df, name, count, types=None, genres=None):
    """anime_recs (similar_anime.py:364-471): cosine of the query anime vs all, query excluded,
    optional Type / Genre filters, top ``count`` by similarity.  Returns (frame, filename)."""
    import torch
    from . import ops
    qid = find_anime_id(name, anime_df)
    pos = np.nonzero(np.asarray(anime_ids) == qid)[0]
    if len(pos) == 0:
        raise ValueError("anime %r (id %d) has no embedding row" % (name, qid))
    q = int(pos[0])
    meta = metadata_by_index(anime_ids, anime_df, syn_df)
    keep = filter_mask(meta, anime_df, types, genres)
    Wh = ops.rownorm(torch.as_tensor(A))
    k = _topk_count(count, "a_query_number", len(anime_ids) - 1)
    idx, sim = ops.cosine_topk(Wh, [q], k, exclude_self=True, keep=keep.astype(np.uint8))
    idx, sim = idx.cpu().numpy()[0], sim.cpu().numpy()[0]
    frame = _similar_anime_rows(meta, idx, sim)
    return frame, clean(name) + ".csv"


# ----------------------------------------------------------------------------------------
# also_liked: "people who liked this also liked ...", from the ratings alone
# ----------------------------------------------------------------------------------------
COOC_MEASURES = ("cosine", "jaccard", "confidence")


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def also_liked_frame(df, anime_df, syn_df, name, count, types=None, genres=None, liked_min_rating=0.0,
                     measure="cosine", shrink=0.0, min_support=1):
    """The anime most often liked together with the query anime: no model takes part.  A user LIKED an anime when
    ``df``'s rating of the pair is at or above ``liked_min_rating`` (0.0 = every rating counts); the similarity of two
    anime is the ``measure`` (cosine, jaccard, confidence) of their liked-by sets (``ops.cooc_scores``), the list the
    exact select's (``ops.rows_topk``: larger first, ties by index) over the anime that pass the optional Type / Genre
    filters and share at least max(1, ``min_support``) users with the query.  Returns (frame, filename): similar_anime's
    columns with the measure as ``Similarity``, then ``Liked_by_both`` (the users who liked both) and ``Liked_by`` (those
    who liked the listed anime).  The anime index is the rating frame's own (order of first appearance)."""
    from . import ops, recs
    measure = str(measure).strip().lower()
    if measure not in COOC_MEASURES:
        raise ValueError("cooc_measure %r is not one of %s" % (measure, ", ".join(COOC_MEASURES)))
    ops.check_cooc(measure, shrink, min_support)
    user_ids, anime_ids = index_tables({}, df)
    qid = find_anime_id(name, anime_df)
    pos = np.nonzero(np.asarray(anime_ids) == qid)[0]
    if len(pos) == 0:
        raise ValueError("anime %r (id %d) has no rating in the main data frame" % (name, qid))
    q = int(pos[0])
    meta = metadata_by_index(anime_ids, anime_df, syn_df)
    keep = filter_mask(meta, anime_df, types, genres)
    ui, ai, r = rating_indices(df, user_ids, anime_ids)
    liked = r.astype(np.float32) >= np.float32(liked_min_rating)
    bits = recs.item_bits(ui[liked], ai[liked], len(user_ids), len(anime_ids))
    k = _topk_count(count, "a_query_number", len(anime_ids) - 1)
    sim, cnt, excl, pop = ops.cooc_scores(bits, len(user_ids), [q], measure, shrink, min_support, count=True, excl=True,
                                          pop=True)
    idx, s = ops.rows_topk(sim, k, keep=keep.astype(np.uint8), wbits=excl)
    idx, s, cnt, pop = _np(idx)[0], _np(s)[0], _np(cnt)[0], _np(pop)
    frame = _similar_anime_rows(meta, idx, s)
    ok = idx >= 0
    frame["Liked_by_both"] = cnt[idx[ok]].astype(np.int64)
    frame["Liked_by"] = pop[idx[ok]].astype(np.int64)
    return frame, clean(name) + "_also_liked.csv"


# ----------------------------------------------------------------------------------------
# content_recs: lists from all_anime.csv's own columns, for titles nobody has rated too
# ----------------------------------------------------------------------------------------
CONTENT_SHARED_TOKENS = 5    # tokens named per listed anime in Shared_tokens


def content_universe(anime_df):
    """The item index of the content components: every anime of all_anime.csv, in the frame's order."""
    return anime_df.drop_duplicates("anime_id")["anime_id"].to_numpy()


def _content_checks(columns, weight="rating"):
    from . import recs
    recs.content_history_weights([], weight)
    return recs.check_content_fit(columns)[0]


def content_similar_frame(anime_df, syn_df, name, count, types=None, genres=None, columns=None):
    """The anime closest to the query anime by content: no model and no rating takes part, so the query and the listed
    anime may have no rating at all.  The items are every row of ``anime_df``; their TF-IDF rows come from ``columns``
    (default CONTENT_COLUMNS; ``recs.content_fit``), the list from ``recs.content_similar`` over the anime that pass the
    optional Type / Genre filters.  Returns (frame, filename): similar_anime's columns with the content cosine as
    ``Similarity``, then ``Shared_tokens``: the (at most CONTENT_SHARED_TOKENS) tokens both rows carry with the largest
    product of weights, joined by " | "."""
    from . import recs
    columns = _content_checks(CONTENT_COLUMNS if columns is None else columns)
    anime_ids = content_universe(anime_df)
    qid = find_anime_id(name, anime_df)
    q = int(np.nonzero(anime_ids == qid)[0][0])
    meta = metadata_by_index(anime_ids, anime_df, syn_df)
    keep = filter_mask(meta, anime_df, types, genres)
    fit = recs.content_fit(meta, columns)
    k = _topk_count(count, "a_query_number", len(anime_ids) - 1)
    idx, s = recs.content_similar(fit, [q], k, keep.astype(np.uint8))
    idx, s = _np(idx)[0], _np(s)[0]
    frame = _similar_anime_rows(meta, idx, s)
    off, ti, tw = _np(fit["tok_offsets"]), _np(fit["tok_idx"]), _np(fit["tok_w"])
    own = {int(v): float(w) for v, w in zip(ti[off[q]:off[q + 1]], tw[off[q]:off[q + 1]])}
    shared = []
    for j in idx[idx >= 0]:
        both = [(-own[int(v)] * float(w), int(v)) for v, w in zip(ti[off[j]:off[j + 1]], tw[off[j]:off[j + 1]])
                if int(v) in own]
        shared.append(_SEP.join(fit["vocab"][v] for _, v in sorted(both)[:CONTENT_SHARED_TOKENS]))
    frame["Shared_tokens"] = shared
    return frame, clean(name) + "_content.csv"


def content_recs_frame(df, anime_df, syn_df, user_id, n_recs, types=None, genres=None, columns=None, weight="rating",
                       min_rating=0.0):
    """One user's content-based list among the anime they have not rated: the items are every row of ``anime_df``, the
    profile the weighted mean of the TF-IDF rows (``recs.content_fit`` over ``columns``, default CONTENT_COLUMNS) of the
    user's ratings in ``df`` at or above ``min_rating`` (compared in fp32), weighted per ``weight``
    (``recs.content_history_weights``); the list is ``recs.content_topk``'s over the unrated anime that pass the optional
    Type / Genre filters.  Returns model_recs_frame's columns with ``Content_score`` in the place of ``Prediction``.
    ValueError before any GPU use for an unknown column or weight and for a user without ratings."""
    from . import recs
    columns = _content_checks(CONTENT_COLUMNS if columns is None else columns, weight)
    anime_ids = content_universe(anime_df)
    mine = df[df.user_id == int(user_id)]
    if not len(mine):
        raise ValueError("user id %r has no rating in the main data frame" % (user_id,))
    pos = pd.Series(np.arange(len(anime_ids)), index=anime_ids).reindex(mine.anime_id.to_numpy()).to_numpy()
    r = mine.rating.to_numpy().astype(np.float32)
    take = ~np.isnan(pos) & (r >= np.float32(min_rating))
    hist, r = pos[take].astype(np.int32), r[take]
    meta, bits = _filter_bits(anime_ids, anime_df, syn_df, types, genres)
    bits = bits | _blocked_bits(~unwatched_mask(df, anime_ids, user_id)).view(np.int32)
    fit = recs.content_fit(meta, columns)
    k = _topk_count(n_recs, "model_num_recs", len(anime_ids))
    idx, s = recs.content_topk(fit, [0, len(hist)], hist, recs.content_history_weights(r, weight), k, bits)
    idx, s = _np(idx)[0], _np(s)[0]
    return _model_recs_rows(meta, idx, s).rename(columns={"Prediction": "Content_score"})


# ----------------------------------------------------------------------------------------
# ease_recs: lists from the closed-form linear item-item model, from the ratings alone
# ----------------------------------------------------------------------------------------
def _ease_fit_frame(df, liked_min_rating, reg, neighbours):
    """(fit, user_ids, anime_ids, (ui, ai, r)): ``recs.ease_fit`` on the rating frame's own index (order of first
    appearance), the checks that need no GPU first"""
    from . import ops, recs
    reg, neighbours = ops.check_ease(reg, neighbours)
    user_ids, anime_ids = index_tables({}, df)
    ui, ai, r = rating_indices(df, user_ids, anime_ids)
    fit = recs.ease_fit(ui, ai, r, len(user_ids), len(anime_ids), liked_min_rating, reg, neighbours)
    return fit, user_ids, anime_ids, (ui, ai, r)


def ease_stats(fit):
    """What the ease_recs artifacts record about the fit"""
    return {"reg": float(fit["reg"]), "n_items": int(fit["n_items"]), "liked_pairs": int(fit["n_liked"]),
            "neighbours": int(fit["neighbours"]), "liked_min_rating": float(fit["liked_min_rating"])}


def ease_similar_frame(df, anime_df, syn_df, name, count, types=None, genres=None, liked_min_rating=0.0, reg=500.0,
                       neighbours=0):
    """The anime with the largest weights in the query anime's row of the EASE item-item matrix (what liking the query
    adds most to): no model takes part.  A user LIKED an anime when ``df``'s rating of the pair is at or above
    ``liked_min_rating``; the fit is ``recs.ease_fit`` (``reg`` = 500 is the paper's value for a data set of about this
    many users, not tuned on this data), the list ``recs.ease_similar``'s over the anime that pass the optional Type /
    Genre filters.  Returns (frame, filename, stats): similar_anime's columns with the weight as ``Similarity``."""
    from . import ops, recs
    ops.check_ease(reg, neighbours)
    qid = find_anime_id(name, anime_df)
    pos = np.nonzero(np.asarray(index_tables({}, df)[1]) == qid)[0]
    if len(pos) == 0:
        raise ValueError("anime %r (id %d) has no rating in the main data frame" % (name, qid))
    fit, user_ids, anime_ids, _ = _ease_fit_frame(df, liked_min_rating, reg, neighbours)
    meta = metadata_by_index(anime_ids, anime_df, syn_df)
    keep = filter_mask(meta, anime_df, types, genres)
    k = _topk_count(count, "a_query_number", len(anime_ids) - 1)
    idx, s = recs.ease_similar(fit, [int(pos[0])], k, keep.astype(np.uint8))
    return _similar_anime_rows(meta, _np(idx)[0], _np(s)[0]), clean(name) + "_ease.csv", ease_stats(fit)


def ease_recs_frame(df, anime_df, syn_df, user_id, n_recs, types=None, genres=None, liked_min_rating=0.0, reg=500.0,
                    neighbours=0):
    """One user's EASE list among the anime they have not rated: the history is the user's ratings in ``df`` at or above
    ``liked_min_rating`` (compared in fp32) with weight 1, scored through ``recs.ease_fit``'s weights (the truncated
    model's, with ``neighbours`` > 0); the list is the exact select's over the unrated anime that pass the optional Type /
    Genre filters.  Returns (frame, stats): model_recs_frame's columns with ``Ease_score`` in the place of
    ``Prediction``.  ValueError before any GPU use for a bad ``reg`` or ``neighbours`` and a user without ratings."""
    from . import ops, recs
    ops.check_ease(reg, neighbours)
    if not (df.user_id == int(user_id)).any():
        raise ValueError("user id %r has no rating in the main data frame" % (user_id,))
    fit, user_ids, anime_ids, (ui, ai, r) = _ease_fit_frame(df, liked_min_rating, reg, neighbours)
    row = int(np.nonzero(np.asarray(user_ids) == int(user_id))[0][0])
    off, hist, _ = recs.history_csr(ui, ai, r, [row], min_rating=liked_min_rating)
    meta, bits = _filter_bits(anime_ids, anime_df, syn_df, types, genres)
    bits = bits | _blocked_bits(~unwatched_mask(df, anime_ids, user_id)).view(np.int32)
    k = _topk_count(n_recs, "model_num_recs", len(anime_ids))
    source = recs.itemknn_rows_source(fit["knn"], off, hist) if fit["neighbours"] else recs.ease_rows_source(fit, off, hist)
    idx, s = recs.rows_topk_batched(source, 1, k, bits, what="ease_recs")
    return _model_recs_rows(meta, _np(idx)[0], _np(s)[0]).rename(columns={"Prediction": "Ease_score"}), ease_stats(fit)


# ----------------------------------------------------------------------------------------
# rp3_recs: lists from the three-step random walk with a popularity penalty, from the ratings alone
# ----------------------------------------------------------------------------------------
def _rp3_fit_frame(df, liked_min_rating, alpha, beta, neighbours):
    """(fit, user_ids, anime_ids, (ui, ai, r)): ``recs.rp3_fit`` on the rating frame's own index (order of first
    appearance), the checks that need no GPU first"""
    from . import recs
    alpha, beta, neighbours = recs.check_rp3(alpha, beta, neighbours)
    user_ids, anime_ids = index_tables({}, df)
    ui, ai, r = rating_indices(df, user_ids, anime_ids)
    fit = recs.rp3_fit(ui, ai, r, len(user_ids), len(anime_ids), liked_min_rating, alpha, beta, neighbours)
    return fit, user_ids, anime_ids, (ui, ai, r)


def rp3_stats(fit):
    """What the rp3_recs artifacts record about the fit"""
    return {"alpha": float(fit["alpha"]), "beta": float(fit["beta"]), "neighbours": int(fit["neighbours"]),
            "n_items": int(fit["n_items"]), "liked_pairs": int(fit["n_liked"]), "scale": float(fit["scale"]),
            "liked_min_rating": float(fit["liked_min_rating"])}


def rp3_similar_frame(df, anime_df, syn_df, name, count, types=None, genres=None, liked_min_rating=0.0, alpha=1.0,
                      beta=0.3, neighbours=100):
    """The anime with the largest weights in the query anime's row of the RP3beta item-item matrix (where a three-step
    walk from the query ends most often, popular endpoints penalised): no model takes part.  A user LIKED an anime when
    ``df``'s rating of the pair is at or above ``liked_min_rating``; the fit is ``recs.rp3_fit`` (alpha = 1, beta = 0.3
    and 100 neighbours are common values from the literature, not tuned on this data), the list ``recs.rp3_similar``'s
    over the anime that pass the optional Type / Genre filters.  Returns (frame, filename, stats): similar_anime's
    columns with the weight as ``Similarity``."""
    from . import recs
    recs.check_rp3(alpha, beta, neighbours)
    qid = find_anime_id(name, anime_df)
    pos = np.nonzero(np.asarray(index_tables({}, df)[1]) == qid)[0]
    if len(pos) == 0:
        raise ValueError("anime %r (id %d) has no rating in the main data frame" % (name, qid))
    fit, user_ids, anime_ids, _ = _rp3_fit_frame(df, liked_min_rating, alpha, beta, neighbours)
    meta = metadata_by_index(anime_ids, anime_df, syn_df)
    keep = filter_mask(meta, anime_df, types, genres)
    k = _topk_count(count, "a_query_number", len(anime_ids) - 1)
    idx, s = recs.rp3_similar(fit, [int(pos[0])], k, keep.astype(np.uint8))
    return _similar_anime_rows(meta, _np(idx)[0], _np(s)[0]), clean(name) + "_rp3.csv", rp3_stats(fit)


def rp3_recs_frame(df, anime_df, syn_df, user_id, n_recs, types=None, genres=None, liked_min_rating=0.0, alpha=1.0,
                   beta=0.3, neighbours=100):
    """One user's RP3beta list among the anime they have not rated: the history is the user's ratings in ``df`` at or
    above ``liked_min_rating`` (compared in fp32) with weight 1, scored through ``recs.rp3_fit``'s weights; the list is
    the exact select's over the unrated anime that pass the optional Type / Genre filters.  Returns (frame, stats):
    model_recs_frame's columns with ``Rp3_score`` in the place of ``Prediction``.  ValueError before any GPU use for a
    bad ``alpha``, ``beta`` or ``neighbours`` and a user without ratings."""
    from . import recs
    recs.check_rp3(alpha, beta, neighbours)
    if not (df.user_id == int(user_id)).any():
        raise ValueError("user id %r has no rating in the main data frame" % (user_id,))
    fit, user_ids, anime_ids, (ui, ai, r) = _rp3_fit_frame(df, liked_min_rating, alpha, beta, neighbours)
    row = int(np.nonzero(np.asarray(user_ids) == int(user_id))[0][0])
    off, hist, _ = recs.history_csr(ui, ai, r, [row], min_rating=liked_min_rating)
    meta, bits = _filter_bits(anime_ids, anime_df, syn_df, types, genres)
    bits = bits | _blocked_bits(~unwatched_mask(df, anime_ids, user_id)).view(np.int32)
    k = _topk_count(n_recs, "model_num_recs", len(anime_ids))
    idx, s = recs.rows_topk_batched(recs.rp3_rows_source(fit, off, hist), 1, k, bits, what="rp3_recs")
    return _model_recs_rows(meta, _np(idx)[0], _np(s)[0]).rename(columns={"Prediction": "Rp3_score"}), rp3_stats(fit)


# ----------------------------------------------------------------------------------------
# onboarding: which anime to show a newcomer, from the ratings alone
# ----------------------------------------------------------------------------------------
ONBOARD_STRATEGIES = ("coverage", "popularity")


def onboarding_frame(df, anime_df, syn_df, count, depth=3, strategy="coverage", types=None, genres=None, max_ratings=0,
                     holdout=0.2, seed=0):
    """The ``count`` anime to ask a newcomer about: no model takes part.  ``strategy="coverage"``: the greedy
    maximum-coverage list (``recs.onboarding_list``) — each anime is the one the most users who know fewer than ``depth``
    of the list so far have rated; ``"popularity"``: the most rated anime.  Only anime that pass the optional Type /
    Genre filters are listed.  ``max_ratings > 0`` restricts the population to users with at most that many ratings in
    ``df`` (a newcomer resembles a light user); 0 means everyone.  A share ``holdout`` of the population (a fixed
    ``default_rng(seed)`` permutation) takes no part in the picking and is what the list is judged on.  Returns (frame,
    summary): similar_anime's metadata columns without ``Similarity``, then ``Rated_by`` (raters among all users),
    ``New_reach`` (the pick's gain: pick users it reached who were still below their depth) and ``Reach_share`` (the
    running sum of the gains over greedy depth x pick users: the share of the best possible the list has reached; the
    greedy depth is ``depth`` for coverage and ``count`` for popularity).  ``summary`` holds the settings and, under
    "coverage" and "popularity", the figures of the chosen strategy AND of the other one on the same split.  The anime
    index is the rating frame's own (order of first appearance)."""
    from . import ops, recs
    strategy = str(strategy).strip().lower()
    if strategy not in ONBOARD_STRATEGIES:
        raise ValueError("onboard_strategy %r is not one of %s" % (strategy, ", ".join(ONBOARD_STRATEGIES)))
    max_ratings = int(max_ratings)
    if max_ratings < 0:
        raise ValueError("onboard_max_ratings must be >= 0 (got %d)" % max_ratings)
    user_ids, anime_ids = index_tables({}, df)
    m = _topk_count(count, "onboard_number", len(anime_ids))
    m, depth = ops.check_cover(m, depth)[0], int(depth)
    meta = metadata_by_index(anime_ids, anime_df, syn_df)
    keep = filter_mask(meta, anime_df, types, genres)
    ui, ai, _ = rating_indices(df, user_ids, anime_ids)
    n_users, n_anime = len(user_ids), len(anime_ids)
    population = None
    if max_ratings > 0:
        population = np.bincount(ui, minlength=n_users) <= max_ratings
    bits = recs.item_bits(ui, ai, n_users, n_anime)
    lists = {s: recs.onboarding_list(ui, ai, n_users, n_anime, m, depth, s, population, keep.astype(np.uint8), holdout,
                                     seed, bits=bits)
             for s in (strategy,) + tuple(s for s in ONBOARD_STRATEGIES if s != strategy)}
    res = lists[strategy]
    idx = res["pick"]
    ok = idx >= 0
    frame = _similar_anime_rows(meta, idx, np.zeros(len(idx), np.float32)).drop(columns=["Similarity"])
    frame["Rated_by"] = res["rated_by"][ok].astype(np.int64)
    frame["New_reach"] = res["gain"][ok].astype(np.int64)
    best = res["greedy_depth"] * res["pick_users"]["users"]
    frame["Reach_share"] = np.cumsum(res["gain"][ok].astype(np.int64)) / float(best) if best else np.nan
    summary = {"strategy": strategy, "count": m, "depth": depth, "max_ratings": max_ratings, "holdout": float(holdout),
               "seed": int(seed), "population": res["pick_users"]["users"] + res["holdout_users"]["users"]}
    for s, r in lists.items():
        summary[s] = {"picks": r["picks"], "pick_users": r["pick_users"], "holdout_users": r["holdout_users"]}
    return frame, summary


# ----------------------------------------------------------------------------------------
# similar_users
# ----------------------------------------------------------------------------------------
def fave_anime(df, anime_df, user_id, num_faves, tv_only):
    """get_fave_anime (similar_users.py:203-256): top-rated anime of a user, narrowed to the
    highest watched fraction, optionally ordered by episode count; returned as the reference's
    ``str(list)[1:-1]`` text."""
    f = df[df.user_id == user_id]
    if len(f) == 0:
        return ""
    f = f[f.rating == f.rating.max()].copy()
    meta = anime_df.drop_duplicates("anime_id").set_index("anime_id")
    f["name"] = meta["Name"].reindex(f.anime_id).to_numpy()
    f["episodes"] = pd.to_numeric(meta["Episodes"].reindex(f.anime_id), errors="coerce").to_numpy(np.float32)
    if "watched_episodes" in f.columns:
        f["percent"] = f["watched_episodes"] / f["episodes"]
        f = f[f.percent == f.percent.max()] if f.percent.notna().any() else f
    if tv_only:
        f = f.sort_values(by="episodes", ascending=False)
    return str(f["name"].tolist()[: int(num_faves)])[1:-1]


def fave_anime_many(df, anime_df, user_ids, num_faves, tv_only):
    """fave_anime of every listed user from one pass over the rating frame (one isin filter and a groupby)
    instead of a full-frame filter per user: the same strings, in the order of `user_ids`."""
    ids = list(user_ids)
    f = df[df.user_id.isin(ids)]
    if len(f) == 0:
        return ["" for _ in ids]
    f = f[f.rating == f.groupby("user_id").rating.transform("max")].copy()
    meta = anime_df.drop_duplicates("anime_id").set_index("anime_id")
    f["name"] = meta["Name"].reindex(f.anime_id).to_numpy()
    f["episodes"] = pd.to_numeric(meta["Episodes"].reindex(f.anime_id), errors="coerce").to_numpy(np.float32)
    if "watched_episodes" in f.columns:
        f["percent"] = f["watched_episodes"] / f["episodes"]
        top = f.groupby("user_id").percent.transform("max")
        has = f.percent.notna().groupby(f.user_id).transform("any")
        f = f[~has | (f.percent == top)]
    out = {}
    for u, g in f.groupby("user_id", sort=False):
        if tv_only:
            g = g.sort_values(by="episodes", ascending=False)
        out[u] = str(g["name"].tolist()[: int(num_faves)])[1:-1]
    return [out.get(u, "") for u in ids]


def similar_users_frame(U, user_ids, df, anime_df, user_id, n_users, num_faves, tv_only):
    """find_similar_users (similar_users.py:262-314): the n most similar users (query dropped),
    descending similarity, with each neighbour's favourite anime."""
    import torch
    from . import ops
    pos = np.nonzero(np.asarray(user_ids) == int(user_id))[0]
    if len(pos) == 0:
        raise ValueError("user id %r has no embedding row" % (user_id,))
    Uh = ops.rownorm(torch.as_tensor(U))
    k = _topk_count(n_users, "id_query_number", len(user_ids) - 1)
    idx, sim = ops.cosine_topk(Uh, [int(pos[0])], k, exclude_self=True)
    idx, sim = idx.cpu().numpy()[0], sim.cpu().numpy()[0]
    ok = idx >= 0
    ids = np.asarray(user_ids)[idx[ok]]
    frame = pd.DataFrame({"similar_users": ids, "similarity": sim[ok],
                          "favorite_animes": fave_anime_many(df, anime_df, ids, num_faves, tv_only)})
    fn = "User_" + str(user_id).translate({ord(c): None for c in string.whitespace}) + ".csv"
    return frame, fn


# ----------------------------------------------------------------------------------------
# model_recs
# ----------------------------------------------------------------------------------------
def _blocked_bits(blocked):
    """One row of watched-bit words ([1, ceil(n_anime/32)] uint32) with the bits of the anime ``blocked`` marks set:
    the mask predict_topk takes for anime a list must not hold."""
    bits = np.zeros((1, (len(blocked) + 31) // 32), np.uint32)
    nz = np.nonzero(blocked)[0]
    np.bitwise_or.at(bits[0], nz >> 5, (np.uint32(1) << (nz & 31).astype(np.uint32)))
    return bits


def _filter_bits(anime_ids, anime_df, syn_df, types, genres):
    """(meta, bits): the metadata by index and, as blocked-bit words (int32), the anime the Type / Genre filters (and a
    missing all_anime.csv row) keep out of a list."""
    meta = metadata_by_index(anime_ids, anime_df, syn_df)
    return meta, _blocked_bits(~filter_mask(meta, anime_df, types, genres)).view(np.int32)


def _candidates(U, A, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs, types, genres, row=None):
    """The candidate stage of the one-user lists (model_recs, explain_recs, diverse_recs, calibrated_recs):
    (row, meta, bits, tU, tA, k) — the user's row of ``U`` (``row`` when the caller has looked it up), the metadata by
    index, the blocked-bit words (int32) of the anime the user has rated or the filters refuse, the two tables on the
    device and the clamped list length."""
    import torch
    if row is None:
        pos = np.nonzero(np.asarray(user_ids) == int(user_id))[0]
        if len(pos) == 0:
            raise ValueError("user id %r has no embedding row" % (user_id,))
        row = int(pos[0])
    meta, bits = _filter_bits(anime_ids, anime_df, syn_df, types, genres)
    bits = bits | _blocked_bits(~unwatched_mask(df, anime_ids, user_id)).view(np.int32)
    tU, tA = torch.as_tensor(U).cuda(), torch.as_tensor(A).cuda()
    return row, meta, bits, tU, tA, _topk_count(n_recs, "model_num_recs", len(anime_ids))


def _model_recs_rows(meta, idx, p):
    """The model_recs frame (model_recs.py:451-456) of one user's top-k: ``idx`` anime indices (-1 padded) with
    their predicted ratings ``p``, metadata from ``meta`` (metadata_by_index)."""
    ok = idx >= 0
    rows = meta.iloc[idx[ok]]
    return pd.DataFrame({
        "Name": rows["Name"].to_numpy(), "Prediction": p[ok], "Genres": rows["Genres"].to_numpy(),
        "Source": rows["Source"].to_numpy(), "anime_id": rows["anime_id"].to_numpy(),
        "Sypnopsis": rows["Sypnopsis"].to_numpy(), "Episodes": rows["Episodes"].to_numpy(),
        "Japanese name": rows["japanese_name"].to_numpy(), "Studios": rows["Studios"].to_numpy(),
        "Premiered": rows["Premiered"].to_numpy(), "Score": rows["Score"].to_numpy(),
        "Type": rows["Type"].to_numpy()})


def model_recs_frame(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs,
                     types=None, genres=None):
    """recommendations (model_recs.py:373-456): predicted rating of every unwatched, indexed
    anime for one user, Type / Genre filters, descending prediction, first ``n_recs``."""
    meta, idx, p, _ = _model_recs_topk(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs, types, genres)
    return _model_recs_rows(meta, idx, p)


def _model_recs_topk(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs, types, genres):
    """model_recs_frame's list before it becomes a frame: (meta, idx, p, tA) — the metadata by index, the anime indices
    (-1 padded) with their predicted ratings on the host, and the anime table on the device."""
    from . import ops
    row, meta, bits, tU, tA, k = _candidates(U, A, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs, types, genres)
    idx, p = ops.predict_topk(tU, tA, head, [row], k, bits)
    return meta, idx.cpu().numpy()[0], p.cpu().numpy()[0], tA


# ----------------------------------------------------------------------------------------
# explain_recs: model_recs with the user's own ratings that put each anime in the list
# ----------------------------------------------------------------------------------------
EXPLAIN_WEIGHTS = ("rating", "similarity")
EXPLAIN_MAX_COUNT = 8    # ANIREC_EXPLAIN_MAX_M


def explain_recs_frame(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs,
                       types=None, genres=None, count=3, weight="rating", min_rating=0.0):
    """model_recs_frame with a reason beside every row (``recs.explain_topk``): the rating sees an anime
    only through the cosine of its row with the user's, so for a listed anime the ``count`` anime of the user's own
    ratings (those at or above ``min_rating``, in the frame's order) with the largest rating * cosine to it
    (``weight`` = ``rating``) or the largest cosine alone (``similarity``).  A list longer than
    anirec_explain_max_k(width) is explained in column blocks of that many (a slot's picks do not depend on the others).
    The frame has model_recs_frame's columns, the same values, then for r = 1 .. count ``Because_r`` (the anime's
    Name), ``Because_r_rating`` (the user's rating of it as the frame holds it), ``Because_r_similarity`` and
    ``Because_r_contribution``; the four cells are empty where the history has no r-th pick or its contribution is
    not > 0."""
    import torch
    from . import _lib, ops, recs
    count = int(count)
    if not 1 <= count <= EXPLAIN_MAX_COUNT:
        raise ValueError("explain_recs: count = %d must be in 1 .. %d" % (count, EXPLAIN_MAX_COUNT))
    if str(weight).strip().lower() not in EXPLAIN_WEIGHTS:
        raise ValueError("explain_recs: weight %r is not one of %s" % (weight, ", ".join(EXPLAIN_WEIGHTS)))
    min_rating = float(min_rating)
    if not 0.0 <= min_rating <= 1.0:
        raise ValueError("explain_recs: min_rating = %r must be in [0, 1]" % (min_rating,))
    meta, idx, p, tA = _model_recs_topk(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs, types, genres)
    frame = _model_recs_rows(meta, idx, p)
    sub = df[df.user_id == int(user_id)]
    arow = pd.Index(np.asarray(anime_ids)).get_indexer(sub.anime_id.to_numpy())
    raw = sub.rating.to_numpy()[arow >= 0]
    offsets, hist_idx, hist_rating = recs.history_csr(np.zeros(len(raw), np.int64), arow[arow >= 0], raw, [0], min_rating)
    raw = raw[raw.astype(np.float32) >= np.float32(min_rating)]          # history_csr's own filter: aligned with the CSR
    assert len(raw) == len(hist_idx)
    What = ops.rownorm(tA, device=tA.device)
    step = _lib.explain_max_k(What.shape[1])
    lists = torch.as_tensor(idx[None, :], device=What.device)
    outs = [recs.explain_topk(What, lists[:, c:c + step], offsets, hist_idx, hist_rating, m=count, weight=weight)
            for c in range(0, lists.shape[1], step)]
    pos, sim, contrib, hist_row = (torch.cat(t, dim=1)[0].cpu().numpy()[idx >= 0] for t in zip(*outs))
    names = meta["Name"].to_numpy()
    for r in range(count):
        ok = (pos[:, r] >= 0) & (contrib[:, r] > 0)
        at = np.where(ok, pos[:, r], 0)
        frame["Because_%d" % (r + 1)] = np.where(ok, names[np.where(ok, hist_row[:, r], 0)], None)
        frame["Because_%d_rating" % (r + 1)] = np.where(ok, raw[at], np.nan) if len(raw) else np.nan
        frame["Because_%d_similarity" % (r + 1)] = np.where(ok, sim[:, r], np.float32(np.nan))
        frame["Because_%d_contribution" % (r + 1)] = np.where(ok, contrib[:, r], np.float32(np.nan))
    return frame


# ----------------------------------------------------------------------------------------
# clusters: the table as a whole — taste communities of the users, micro-genres of the anime
# ----------------------------------------------------------------------------------------
CLUSTER_TABLES = ("anime", "user")
CLUSTER_PERCENTILE = 80.0    # a user's favourites, as user_prefs takes them
CLUSTERS_COLUMNS = ["cluster", "size", "mean_similarity", "top_members", "top_genres"]
_SEP = " | "


def cluster_table_name(table):
    t = str(table).strip().lower()
    if t not in CLUSTER_TABLES:
        raise ValueError("clusters: table %r is not one of %s" % (table, ", ".join(CLUSTER_TABLES)))
    return t


def cluster_genre_counts(table, meta, n_rows, fav_bits=None):
    """(names, counts int64 [n_rows, len(names)]) of the rows of a clustered table: for ``anime`` the Genres tokens an
    anime carries (``category_table``), for ``user`` the genre profile of the user's favourites (``recs.fave_profile``
    over ``fav_bits``, ``favourite_bits`` output)."""
    from . import recs
    names, bits = category_table(meta, "Genres")
    if not names:
        return names, np.zeros((n_rows, 0), np.int64)
    if cluster_table_name(table) == "anime":
        flags = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :len(names)]
        return names, flags.astype(np.int64)
    if fav_bits is None:
        raise ValueError("clusters: the user table's genres need the users' favourite bits")
    return names, recs.fave_profile(fav_bits, bits, len(names)).cpu().numpy().astype(np.int64)


def clusters_frame(fit, table, ids, meta, top=10, n_genres=5, fav_bits=None):
    """One row per cluster of a ``recs.cluster_rows`` result on the ``anime`` or ``user`` table (``ids``: the table's
    index -> id array; ``meta``: ``metadata_by_index``): ``cluster``, ``size``, ``mean_similarity`` (the members' mean
    cosine to the centroid, float64 on the host; empty for an empty cluster), ``top_members`` (the ``top`` members
    nearest the centroid, nearest first, ties to the lower row: anime Names, user ids; joined by " | ") and
    ``top_genres`` (the ``n_genres`` leading genres as "Genre (count)": for anime the members' genre counts, for users
    the members' summed favourite profiles)."""
    table = cluster_table_name(table)
    top = int(top)
    if top < 1:
        raise ValueError("clusters: top = %d must be >= 1" % top)
    a = fit["assign"].cpu().numpy()
    sim = fit["sim"].cpu().numpy().astype(np.float64)
    k = int(fit["C"].shape[0])
    ids = np.asarray(ids)
    if len(a) != len(ids):
        raise ValueError("clusters: %d assignments for a table of %d ids" % (len(a), len(ids)))
    names, counts = cluster_genre_counts(table, meta, len(ids), fav_bits)
    label = meta["Name"].to_numpy() if table == "anime" else None
    rows = []
    for c in range(k):
        members = np.flatnonzero(a == c)
        order = members[np.lexsort((members, -sim[members]))][:top]
        if table == "anime":
            shown = [str(label[i]) if isinstance(label[i], str) else str(ids[i]) for i in order]
        else:
            shown = [str(ids[i]) for i in order]
        tally = counts[members].sum(axis=0) if len(names) else np.zeros(0, np.int64)
        lead = [g for g in np.lexsort((np.arange(len(names)), -tally))[:int(n_genres)] if tally[g] > 0]
        rows.append({"cluster": c, "size": len(members),
                     "mean_similarity": float(sim[members].mean()) if len(members) else np.nan,
                     "top_members": _SEP.join(shown),
                     "top_genres": _SEP.join("%s (%d)" % (names[g], tally[g]) for g in lead)})
    return pd.DataFrame(rows, columns=CLUSTERS_COLUMNS)


def cluster_assignments_frame(fit, table, ids):
    """id, cluster, similarity of every row of the clustered table: ``anime_id`` / ``user_id``, ``cluster`` (-1 for a
    row without one: a zero embedding row), ``similarity`` (its cosine to the cluster's centroid, fp32)."""
    table = cluster_table_name(table)
    return pd.DataFrame({table + "_id": np.asarray(ids), "cluster": fit["assign"].cpu().numpy(),
                         "similarity": fit["sim"].cpu().numpy()})


def cluster_query_row(table, query, user_ids, anime_ids, anime_df):
    """The table row of a ``cluster_query``: for the anime table an anime id (an integer) or a title (resolved as
    similar_anime resolves it), for the user table a user id."""
    table = cluster_table_name(table)
    q = str(query).strip()
    try:
        num = int(q)
    except ValueError:
        num = None
    if table == "user":
        if num is None:
            raise ValueError("clusters: cluster_query %r is not a user id" % (query,))
        return user_index(user_ids, num)
    aid = num if num is not None and num in set(np.asarray(anime_ids).tolist()) else find_anime_id(q, anime_df)
    pos = np.nonzero(np.asarray(anime_ids) == aid)[0]
    if len(pos) == 0:
        raise ValueError("clusters: anime %r is not in the model's anime table" % (query,))
    return int(pos[0])


# ----------------------------------------------------------------------------------------
# embedding_map: a two-dimensional picture of a table (exact t-SNE)
# ----------------------------------------------------------------------------------------
MAP_MAX_ROWS = 50000     # --map_max_rows: a larger table is sampled by the seed


def map_sample(n_rows, max_rows, seed, always=None):
    """The table rows a map is drawn from, ascending: all of them when ``max_rows`` is 0 or the table has no more,
    else ``max_rows`` rows drawn without replacement by ``np.random.default_rng(seed)`` (``always``: a row that is in
    the sample whatever the draw, the query's)."""
    n_rows, max_rows = int(n_rows), int(max_rows)
    if max_rows < 0:
        raise ValueError("embedding_map: map_max_rows = %d must not be negative" % max_rows)
    if max_rows == 0 or n_rows <= max_rows:
        return np.arange(n_rows)
    take = np.random.default_rng(seed).choice(n_rows, size=max_rows, replace=False)
    if always is not None and always not in take:
        take[0] = always
    return np.sort(take)


def map_frame(fit, table, ids, meta=None, clusters=None):
    """One row per mapped table row of a ``recs.map_rows`` result on the ``anime`` or ``user`` table (``ids``: the id of
    every mapped row; ``meta``: the rows' ``metadata_by_index`` for the anime table): ``anime_id`` / ``user_id``,
    ``name`` (anime only), ``x``, ``y`` (fp32; empty for a row without a position: a zero embedding row) and
    ``cluster`` (the rows' ``recs.cluster_rows`` assignment where ``clusters`` is one, else -1)."""
    table = cluster_table_name(table)
    Y = fit["Y"].cpu().numpy()
    ids = np.asarray(ids)
    if len(Y) != len(ids):
        raise ValueError("embedding_map: %d positions for %d ids" % (len(Y), len(ids)))
    cols = {table + "_id": ids}
    if table == "anime":
        label = meta["Name"].to_numpy() if meta is not None else [None] * len(ids)
        cols["name"] = [str(label[i]) if isinstance(label[i], str) else str(ids[i]) for i in range(len(ids))]
    cols["x"], cols["y"] = Y[:, 0], Y[:, 1]
    cols["cluster"] = clusters["assign"].cpu().numpy() if clusters is not None else np.full(len(ids), -1, np.int32)
    return pd.DataFrame(cols)


def map_neighbours_on_map(frame, row, k=10):
    """The ``k`` rows of a ``map_frame`` nearest ``row`` ON THE MAP (Euclidean, float64, ties to the lower row; rows
    without a position never): a list of (id, name or None, distance)."""
    xy = frame[["x", "y"]].to_numpy(np.float64)
    d = np.sqrt(((xy - xy[row]) ** 2).sum(axis=1))
    d[row] = np.nan
    order = [i for i in np.lexsort((np.arange(len(d)), d)) if np.isfinite(d[i])][:int(k)]
    idc = frame.columns[0]
    return [(frame[idc].iloc[i].item(), str(frame["name"].iloc[i]) if "name" in frame else None, float(d[i]))
            for i in order]


def map_plot(frame, path, title=None):
    """A PNG scatter of a ``map_frame`` coloured by cluster (matplotlib's Agg backend).  Returns False, having written
    nothing, where matplotlib cannot be imported."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    ok = np.isfinite(frame["x"].to_numpy()) & np.isfinite(frame["y"].to_numpy())
    fig, ax = plt.subplots(figsize=(10, 10))
    ax.scatter(frame["x"][ok], frame["y"][ok], c=frame["cluster"][ok], s=4, cmap="tab20", linewidths=0)
    ax.set_xticks([])
    ax.set_yticks([])
    if title:
        ax.set_title(title)
    fig.savefig(path, dpi=120, bbox_inches="tight")
    plt.close(fig)
    return True


# ----------------------------------------------------------------------------------------
# diverse_recs: model_recs with a greedy MMR re-rank of the best `pool` candidates
# ----------------------------------------------------------------------------------------
def _list_cosines(Wh, idx):
    """The cosine matrix (float64, host) of the listed rows ``idx`` (-1 padding dropped) of the normalised table ``Wh``."""
    rows = Wh[np.asarray(idx[idx >= 0], np.int64)].cpu().numpy().astype(np.float64)
    return rows @ rows.T


def _mean_pairwise(S):
    """Mean of the cosines of the distinct pairs of a list (NaN for a list of fewer than two)."""
    n = len(S)
    return float(S[np.triu_indices(n, 1)].mean()) if n >= 2 else float("nan")


def diverse_recs_frame(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs,
                       types=None, genres=None, pool=100, diversity=0.3):
    """model_recs_frame with the list diversified (``recs.diverse_topk``): the same candidates (unwatched, indexed,
    Type / Genre filters), the ``pool`` best by predicted rating re-ranked greedily with ``lam = 1 - diversity``.
    Returns (frame, stats): model_recs_frame's columns plus ``Max_similarity`` — the largest cosine of the row's anime
    to the rows above it, 0 for the first: the re-rank's own penalty (at diversity 0, where nothing is re-ranked and the
    rows are model_recs_frame's, the same quantity from the host's cosines) — and stats = {"mean_similarity": the mean
    pairwise cosine of the listed anime, "mean_similarity_topk": that of the plain top-k}."""
    from . import ops, recs
    row, meta, bits, tU, tA, k = _candidates(U, A, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs, types, genres)
    idx, p, pen = recs.diverse_topk(tU, tA, head, [row], k, pool, diversity, bits)
    idx, p = idx.cpu().numpy()[0], p.cpu().numpy()[0]
    Wh = ops.rownorm(tA, device=tA.device)
    S = _list_cosines(Wh, idx)
    if pen is None:
        plain, pen = S, np.array([S[i, :i].max() if i else 0.0 for i in range(len(S))], np.float32)
    else:
        plain = _list_cosines(Wh, ops.predict_topk(tU, tA, head, [row], k, bits)[0].cpu().numpy()[0])
        pen = pen.cpu().numpy()[0][idx >= 0]
    frame = _model_recs_rows(meta, idx, p)
    frame["Max_similarity"] = pen
    return frame, {"mean_similarity": _mean_pairwise(S), "mean_similarity_topk": _mean_pairwise(plain)}


# ----------------------------------------------------------------------------------------
# hybrid_recs: model_recs' list from the fused score rows of several systems
# ----------------------------------------------------------------------------------------
def hybrid_recs_frame(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs,
                      types=None, genres=None, systems=("model", "itemknn", "als"), weights=None, method="rrf", rrf_c=60,
                      itemknn=None, als=None, ease=None, rp3=None, bpr=None):
    """model_recs_frame with the list taken from several systems at once (``recs.hybrid_topk``): the same candidates
    (unwatched, indexed, Type / Genre filters), each member of ``systems`` (names of ``recs.HYBRID_SYSTEMS``) scoring
    every anime for the user (``content``, of ``recs.CONTENT_SYSTEMS``, with CONTENT_DEFAULTS and this call's metadata), the
    score rows fused per row under the candidates' mask (``ops.fuse_rows``: ``method`` rrf
    with ``rrf_c``, or minmax; ``weights`` None = all 1) and the best ``n_recs`` taken by the exact select.  The item-kNN
    and ALS members are fitted from ``df`` (ITEMKNN_DEFAULTS / ALS_DEFAULTS overridden by ``itemknn`` / ``als``), the
    ``ease`` member (of ``recs.EASE_SYSTEMS``) likewise (EASE_DEFAULTS overridden by ``ease``), the ``rp3`` member (of
    ``recs.GRAPH_SYSTEMS``) likewise (RP3_DEFAULTS overridden by ``rp3``), the ``bpr`` member (of
    ``recs.PAIRWISE_SYSTEMS``) likewise (BPR_DEFAULTS overridden by ``bpr``), the
    user's history and the liked pairs built as ``evaluate_frame`` builds them; popularity is the rating count.
    Returns (frame, stats): model_recs_frame's columns — ``Prediction`` remains the model's predicted rating of the
    listed anime — plus ``Hybrid_score`` (the fused value) and one ``Rank_<system>`` per member: the 1-based place of the
    anime in that member's own ranking under the same mask (``ops.rows_rank``); stats = {"hybrid_systems",
    "hybrid_weights", "hybrid_method", "hybrid_rrf_c"}.  ValueError before any GPU use for an unknown or repeated system,
    no system, or a weights list of another length."""
    from . import ops, recs
    members, ws, method, rrf_c = recs.check_hybrid(systems, weights, method, rrf_c)
    content = {"meta": metadata_by_index(anime_ids, anime_df, syn_df)} if "content" in members else None
    params = _system_params({"itemknn": itemknn, "als": als, "content": content, "ease": ease, "rp3": rp3, "bpr": bpr},
                            members)
    row, meta, bits, tU, tA, k = _candidates(U, A, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs, types, genres)
    cols = None
    if set(members) - {"model"}:
        cols = rating_indices(df, user_ids, anime_ids) + (len(user_ids), len(anime_ids))
    sources = [_system_source(m, (tU, tA, head), cols, params, [row], tA.device) for m in members]
    rows = [src(0, 1) if callable(src) else src.reshape(1, -1) for src in sources]   # scored once: fused and ranked below
    idx, fused = recs.hybrid_topk([lambda l0, l1, x=x: x[l0:l1] for x in rows], k, ws, method, rrf_c, bits)
    idx, fused = _np(idx)[0], _np(fused)[0]
    ok = idx >= 0
    grid = rows[members.index("model")] if "model" in members else ops.predict_grid(tU, tA, head, [row])
    p = np.full(len(idx), np.nan, np.float32)
    p[ok] = _np(grid)[0][idx[ok]]
    frame = _model_recs_rows(meta, idx, p)
    frame["Hybrid_score"] = fused[ok]
    for m, x in zip(members, rows):
        frame["Rank_" + m] = _np(ops.rows_rank(x, np.zeros(int(ok.sum()), np.int64), idx[ok], bits)).astype(np.int64) + 1
    return frame, {"hybrid_systems": list(members), "hybrid_weights": [float(w) for w in ws], "hybrid_method": method,
                   "hybrid_rrf_c": int(rrf_c)}


# ----------------------------------------------------------------------------------------
# calibrated_recs: model_recs with the list pulled towards the user's own genre (or source) proportions
# ----------------------------------------------------------------------------------------
CALIBRATION_COLUMNS = ("Genres", "Source")


def calibrated_recs_frame(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs,
                          types=None, genres=None, pool=100, calibration=0.5, column="Genres", favorite_percentile=80):
    """model_recs_frame with the list calibrated (``recs.calibrated_topk``): the same candidates
    (unwatched, indexed, Type / Genre filters), the ``pool`` best by predicted rating re-ranked greedily so that the
    tokens of ``column`` (``Genres`` or ``Source``) in the list follow the proportions they have among the user's
    favourites (user_prefs' profile: ratings at or above the ``favorite_percentile`` of the user's own).
    Returns (frame, stats): model_recs_frame's columns plus ``Miscalibration`` — the total variation distance between
    the two token distributions for the list down to and including the row: the re-rank's own penalty (at calibration
    0, where nothing is re-ranked and the rows are model_recs_frame's, ``recs.list_calibration`` of the prefixes) — and
    stats = {"calibration", "pool", "column", "n_favourites", "miscalibration": that of the whole list,
    "miscalibration_topk": that of the plain top-k}."""
    import torch
    from . import ops, recs
    if column not in CALIBRATION_COLUMNS:
        raise ValueError("calibrated_recs: calibration_column %r is not one of %s" % (column, ", ".join(CALIBRATION_COLUMNS)))
    u, meta, bits, tU, tA, k = _candidates(U, A, user_ids, anime_ids, df, anime_df, syn_df, user_id, n_recs, types, genres,
                                           row=user_index(user_ids, user_id))
    names, cat_bits = category_table(meta, column)
    n_cat = len(names)
    if n_cat < 1:
        raise ValueError("calibrated_recs: column %r holds no tokens to calibrate to" % (column,))
    fav = favourite_bits(df, user_ids, anime_ids, favorite_percentile)
    profile = recs.fave_profile(fav, cat_bits, n_cat, users=[u])
    idx, p, pen = recs.calibrated_topk(tU, tA, head, [u], k, pool, calibration, cat_bits, n_cat, profile, bits)

    def prefixes(row):
        """the miscalibration of every prefix of one list (-1 padding dropped), by the list kernel"""
        row = row[row >= 0]
        if len(row) == 0:
            return np.zeros(0, np.float32)
        lists = np.where(np.arange(len(row))[None, :] <= np.arange(len(row))[:, None], row[None, :], -1).astype(np.int32)
        return recs.list_calibration(torch.from_numpy(lists).cuda(), cat_bits, n_cat,
                                     profile.expand(len(row), n_cat))[0].cpu().numpy()

    idx, p = idx.cpu().numpy()[0], p.cpu().numpy()[0]
    if pen is None:
        pen = plain = prefixes(idx)
    else:
        plain = prefixes(ops.predict_topk(tU, tA, head, [u], k, bits)[0].cpu().numpy()[0])
        pen = pen.cpu().numpy()[0][idx >= 0]
    frame = _model_recs_rows(meta, idx, p)
    frame["Miscalibration"] = pen
    last = lambda x: float(x[-1]) if len(x) else float("nan")      # noqa: E731
    return frame, {"calibration": float(calibration), "pool": int(pool), "column": column,
                   "n_favourites": int(len(favourite_indices(fav, u, len(anime_ids)))),
                   "miscalibration": last(pen), "miscalibration_topk": last(plain)}


# ----------------------------------------------------------------------------------------
# group_recs: one list for several users who watch together
# ----------------------------------------------------------------------------------------
GROUP_STRATEGIES = ("mean", "least_misery", "most_pleasure")


def group_label(members):
    """The members of a group as a file name holds them: the ids joined by ``_``; above 8 members the first id and
    how many more."""
    members = [int(u) for u in members]
    if len(members) > 8:
        return "%d_and_%d_more" % (members[0], len(members) - 1)
    return "_".join(str(u) for u in members)


def group_recs_frame(U, A, head, user_ids, anime_ids, df, anime_df, syn_df, members, n_recs, types=None, genres=None,
                     strategy="mean", floor=None):
    """model_recs_frame for a group (``ops.group_topk``): the candidates are the indexed anime no member
    (``members``: user ids, a repeated id counts twice) has rated, under the same Type / Genre filters; they are ranked
    by the ``strategy`` (``mean``, ``least_misery``, ``most_pleasure``) of the members' predicted ratings, and with
    ``floor`` an anime any member rates below it is no candidate.  The frame has model_recs_frame's columns with
    ``Prediction`` the aggregate, then ``Min_prediction``, ``Max_prediction`` and one ``User_<id>`` column per distinct
    member: that member's own predicted rating.  A one-member group gives model_recs_frame's rows."""
    import torch
    from . import ops, recs
    members = [int(u) for u in members]
    if not members:
        raise ValueError("group_recs: the group has no members")
    users, offsets, member_row = recs.group_csr([members], user_ids)
    meta, exclude = _filter_bits(anime_ids, anime_df, syn_df, types, genres)
    uid = np.asarray(user_ids)
    watched = np.concatenate([_blocked_bits(~unwatched_mask(df, anime_ids, uid[r])) for r in users])
    tU, tA = torch.as_tensor(U).cuda(), torch.as_tensor(A).cuda()
    k = _topk_count(n_recs, "model_num_recs", len(anime_ids))
    idx, p, mp = ops.group_topk(tU, tA, head, users, offsets, member_row, k, mode=strategy, floor=floor,
                                watched_bits=watched.view(np.int32), exclude_bits=exclude,
                                member_ratings=True)
    idx, p, mp = idx.cpu().numpy()[0], p.cpu().numpy()[0], mp.cpu().numpy()
    frame = _model_recs_rows(meta, idx, p)
    ok = idx >= 0
    frame["Min_prediction"] = mp[:, ok].min(axis=0)
    frame["Max_prediction"] = mp[:, ok].max(axis=0)
    for e, u in enumerate(members):
        if "User_%d" % u not in frame.columns:
            frame["User_%d" % u] = mp[e, ok]
    return frame


# ----------------------------------------------------------------------------------------
# new_user_recs: users the model was not trained on
# ----------------------------------------------------------------------------------------
def _folded_position(folded, user_id):
    pos = np.nonzero(np.asarray(folded["ids"]) == int(user_id))[0]
    if len(pos) == 0:
        raise ValueError("user id %r is not in the new ratings file" % (user_id,))
    return int(pos[0])


def new_user_recs_frame(model, new_df, anime_df, syn_df, user_id, n_recs, types=None, genres=None, steps=None, lr=None,
                        folded=None):
    """model_recs for a user the model holds no row for: every user of ``new_df`` (``user_id, anime_id, rating`` in
    [0, 1]) is folded in by one ``recs.fold_in_users`` call (or taken from ``folded``, an earlier call's result), then
    the queried user's unwatched anime are ranked by predicted rating under the Type / Genre filters, exactly as
    ``model_recs_frame`` does for a trained row.  Returns (frame with model_recs_frame's columns, folded)."""
    import torch
    from . import ops, recs, weights_io
    if folded is None:
        folded = recs.fold_in_users(model, new_df, steps=recs.FOLD_STEPS if steps is None else int(steps),
                                    lr=recs.FOLD_LR if lr is None else float(lr))
    q = _folded_position(folded, user_id)
    anime_ids = np.asarray(model["anime_ids"])
    meta, bits = _filter_bits(anime_ids, anime_df, syn_df, types, genres)
    n_a = len(anime_ids)
    dev = folded["rows"].device
    watched = folded["watched"][q:q + 1] | torch.as_tensor(bits, device=dev)
    tA = torch.as_tensor(np.ascontiguousarray(model["A"], np.float32), device=dev)
    k = _topk_count(n_recs, "model_num_recs", n_a)
    idx, p = ops.predict_topk(folded["rows"], tA, weights_io.model_head(model), [q], k, watched)
    return _model_recs_rows(meta, idx.cpu().numpy()[0], p.cpu().numpy()[0]), folded


def new_user_neighbours_frame(model, folded, df, anime_df, user_id, n_users, num_faves, tv_only):
    """similar_users for a folded user: the trained users ranked by cosine against the folded row — the folded rows
    are appended to the user table and barred as candidates (``keep`` zero), so only trained users are listed.
    ``df``: the rating frame the favourites of the neighbours are read from.  Returns (similar_users frame, filename)."""
    import torch
    from . import ops
    q = _folded_position(folded, user_id)
    user_ids = np.asarray(model["user_ids"])
    n_old = len(user_ids)
    dev = folded["rows"].device
    table = torch.cat([torch.as_tensor(np.ascontiguousarray(model["U"], np.float32), device=dev), folded["rows"]])
    keep = np.zeros(table.shape[0], np.uint8)
    keep[:n_old] = 1
    k = _topk_count(n_users, "id_query_number", n_old)
    idx, sim = ops.cosine_topk(ops.rownorm(table, device=dev), [n_old + q], k, exclude_self=True, keep=keep)
    idx, sim = idx.cpu().numpy()[0], sim.cpu().numpy()[0]
    ok = idx >= 0
    ids = user_ids[idx[ok]]
    frame = pd.DataFrame({"similar_users": ids, "similarity": sim[ok],
                          "favorite_animes": fave_anime_many(df, anime_df, ids, num_faves, tv_only)})
    fn = "User_" + str(user_id).translate({ord(c): None for c in string.whitespace}) + ".csv"
    return frame, fn


# ----------------------------------------------------------------------------------------
# new_anime: anime the model was not trained on
# ----------------------------------------------------------------------------------------
def _folded_anime_position(folded, anime_id):
    pos = np.nonzero(np.asarray(folded["ids"]) == int(anime_id))[0]
    if len(pos) == 0:
        raise ValueError("anime id %r is not in the new ratings file" % (anime_id,))
    return int(pos[0])


def new_anime_similar_frame(model, folded, anime_df, syn_df, anime_id, count, types=None, genres=None):
    """similar_anime for a folded anime (``recs.fold_in_anime``'s result): the trained anime ranked by cosine against
    the folded row under the Type / Genre filters — the folded rows are appended to the anime table and barred as
    candidates (``keep`` zero), so only trained anime are listed.  Returns (frame with similar_anime_frame's columns,
    filename)."""
    import torch
    from . import ops
    q = _folded_anime_position(folded, anime_id)
    anime_ids = np.asarray(model["anime_ids"])
    n_old = len(anime_ids)
    meta = metadata_by_index(anime_ids, anime_df, syn_df)
    dev = folded["rows"].device
    table = torch.cat([torch.as_tensor(np.ascontiguousarray(model["A"], np.float32), device=dev), folded["rows"]])
    keep = np.zeros(table.shape[0], np.uint8)
    keep[:n_old] = filter_mask(meta, anime_df, types, genres)
    k = _topk_count(count, "a_query_number", n_old)
    idx, sim = ops.cosine_topk(ops.rownorm(table, device=dev), [n_old + q], k, exclude_self=True, keep=keep)
    idx, sim = idx.cpu().numpy()[0], sim.cpu().numpy()[0]
    frame = _similar_anime_rows(meta, idx, sim)
    return frame, "Anime_ID_" + str(int(anime_id)) + "_similar.csv"


def new_anime_audience_frame(model, folded, anime_id, n_users):
    """The trained users with the highest predicted rating of a folded anime among those who have not rated it:
    ``ops.predict_topk`` with the two tables in each other's place (the head sees the rows through their cosine
    alone) and the anime's ``rated`` bits as the mask.  Returns (frame ``user_id, Prediction``, filename)."""
    import torch
    from . import ops, weights_io
    q = _folded_anime_position(folded, anime_id)
    user_ids = np.asarray(model["user_ids"])
    dev = folded["rows"].device
    tU = torch.as_tensor(np.ascontiguousarray(model["U"], np.float32), device=dev)
    k = _topk_count(n_users, "audience_number", len(user_ids))
    idx, p = ops.predict_topk(folded["rows"], tU, weights_io.model_head(model), [q], k, folded["rated"][q:q + 1])
    idx, p = idx.cpu().numpy()[0], p.cpu().numpy()[0]
    ok = idx >= 0
    frame = pd.DataFrame({"user_id": user_ids[idx[ok]], "Prediction": p[ok]})
    return frame, "Anime_ID_" + str(int(anime_id)) + "_audience.csv"


# ----------------------------------------------------------------------------------------
# evaluate
# ----------------------------------------------------------------------------------------
def held_out_targets(table, test_size, min_rating):
    """``recs.held_out_targets``: the one definition of the ranking targets, which trainer.fit's ranking columns read
    too."""
    from . import recs
    return recs.held_out_targets(table, test_size, min_rating)


def _tables_of(model, table):
    """(U, A) of ``model`` as arrays, or a ValueError when its id tables are not the rating table's."""
    U, A = np.asarray(model["U"]), np.asarray(model["A"])
    mu, ma = model.get("user_ids"), model.get("anime_ids")
    same = U.shape[0] == table.n_users and A.shape[0] == table.n_anime
    if same and mu is not None and ma is not None:
        same = np.array_equal(np.asarray(mu), np.asarray(table.user_ids)) and \
            np.array_equal(np.asarray(ma), np.asarray(table.anime_ids))
    if not same:
        raise ValueError("the model's id tables are not the rating table's: the model holds %d users x %d anime, the "
                         "table %d users x %d anime (evaluate a model on the data artifact it was trained on)"
                         % (U.shape[0], A.shape[0], table.n_users, table.n_anime))
    return U, A


BASELINES = ("popularity", "itemknn")
ITEMKNN_DEFAULTS = {"neighbours": 50, "measure": "cosine", "shrink": 0.0, "min_support": 1, "min_rating": 0.0}
# baselines that are fitted by optimisation on the training slice: reported after BASELINES.  ALS_DEFAULTS are the usual
# library defaults with the width moved to the nearest supported one; they have not been tuned on this data.
FITTED_BASELINES = ("als",)
ALS_DEFAULTS = {"factors": 64, "sweeps": 15, "cg_steps": 3, "alpha": 1.0, "reg": 0.01, "min_rating": 0.0, "seed": 0}


# systems that fuse the score rows of others: reported after FITTED_BASELINES.  Equal weights and
# rrf_c = 60 are the literature's defaults (Cormack, Clarke and Buettcher 2009); neither is tuned on this data.
FUSED_BASELINES = ("hybrid",)
HYBRID_DEFAULTS = {"systems": ("model", "itemknn", "als"), "weights": None, "method": "rrf", "rrf_c": 60}
# fused systems whose weights are learned, beside FUSED_BASELINES (which stays as it is) and reported
# after it.  hybrid_tuned: the hybrid's members, method and rrf_c with weights chosen from a grid: equal weights and
# every vector of multiples of 1 / steps with sum 1, the best by ``metric`` on the other folds of users
TUNED_BASELINES = ("hybrid_tuned",)
HYBRID_TUNE_DEFAULTS = {"metric": "ndcg@10", "steps": 10, "folds": 2, "seed": 0}
# the content-based system, beside the constants above (which stay as they are) and reported last: it
# scores from all_anime.csv's columns, so it needs the metadata frame by index (the parameter ``meta``).  The defaults
# are the plain choices (every categorical column, the rating as the weight); none is tuned on this data.
CONTENT_BASELINES = ("content",)
CONTENT_COLUMNS = ("Genres", "Type", "Source", "Studios", "Rating")
CONTENT_DEFAULTS = {"columns": CONTENT_COLUMNS, "weight": "rating", "min_rating": 0.0, "min_df": 1, "max_df": 1.0}
# linear item-item models with a closed-form fit (EASE, Steck 2019), beside the constants above (which
# stay as they are) and reported after CONTENT_BASELINES.  reg = 500 is the paper's value for a data set of about this
# many users; it is not tuned on this data.  neighbours = K > 0 keeps the K largest weights of every row only.
LINEAR_BASELINES = ("ease",)
EASE_DEFAULTS = {"reg": 500.0, "min_rating": 0.0, "neighbours": 0}
# graph / random-walk models (P3alpha, Cooper et al. 2014; RP3beta, Paudel et al. 2017), beside the
# constants above (which stay as they are) and reported after LINEAR_BASELINES.  alpha = 1, beta = 0.3 and 100
# neighbours are common values from the literature; none is tuned on this data.  neighbours = 0 keeps the dense matrix.
GRAPH_BASELINES = ("rp3",)
RP3_DEFAULTS = {"alpha": 1.0, "beta": 0.3, "neighbours": 100, "min_rating": 0.0}
# learned models with a PAIRWISE objective (BPR matrix factorisation, Rendle et al. 2009), beside the
# constants above (which stay as they are) and reported last.  BPR_DEFAULTS are the literature's and the ``implicit``
# library's common values with the width moved to the nearest supported one; none is tuned on this data.
PAIRWISE_BASELINES = ("bpr",)
BPR_DEFAULTS = {"factors": 64, "epochs": 30, "batch": 131072, "lr": 0.05, "reg": 0.01, "tries": 8, "bias": True,
                "min_rating": 0.0, "seed": 0}


def _member_params(defaults, given, what):
    par = dict(defaults)
    for key, v in (given or {}).items():
        if key not in par:
            raise ValueError("%s parameter %r is not one of %s" % (what, key, ", ".join(defaults)))
        par[key] = v
    return par


def _systems():
    """One description per system that scores every anime for a list of users (the names of ``recs.HYBRID_SYSTEMS`` and
    ``recs.CONTENT_SYSTEMS``),
    which evaluate_frame and hybrid_recs_frame both go through: ``defaults`` the parameters a caller may override;
    ``check(par)`` the ValueErrors that need no GPU; ``fit(user, anime, rating, n_users, n_anime, par, device)`` the fit
    from training columns (the model has none: its fit is the caller's (U, A, head)); ``source(fit, users, cols, par)``
    the fit's row source for ``users``, cols = fit's first five arguments."""
    from . import ops, recs

    def itemknn_source(knn, users, cols, par):
        off, hist, _ = recs.history_csr(*cols[:3], users, min_rating=par["min_rating"])
        return recs.itemknn_rows_source(knn, off, hist)

    def content_check(par):
        recs.check_content_fit(par["columns"], par["min_df"], par["max_df"])
        recs.content_history_weights([], par["weight"])
        if par["meta"] is None:
            raise ValueError("the content system scores from the anime metadata: give it the frame by index "
                             "(content={'meta': ...}; evaluate: --anime_df)")

    def content_fit(user, anime, rating, n_users, n_anime, par, device):
        if len(par["meta"]) != int(n_anime):
            raise ValueError("content: the metadata frame holds %d rows, the anime index %d" % (len(par["meta"]), n_anime))
        return recs.content_fit(par["meta"], par["columns"], par["min_df"], par["max_df"], device=device)

    def content_source(fit, users, cols, par):
        off, hist, r = recs.history_csr(*cols[:3], users, min_rating=par["min_rating"])
        w = None if str(par["weight"]).strip().lower() == "one" else recs.content_history_weights(r, par["weight"], off)
        return recs.content_rows_source(fit, off, hist, w)

    def als_fit(user, anime, rating, n_users, n_anime, par, device):
        u, a, r = (recs._host(c) for c in (user, anime, rating))
        liked = r.astype(np.float32) >= np.float32(par["min_rating"])
        return recs.als_fit(u[liked], a[liked], n_users, n_anime, par["factors"], int(par["sweeps"]), par["cg_steps"],
                            par["alpha"], par["reg"], seed=int(par["seed"]), device=device)
    return {
        "model": dict(source=lambda tables, users, cols, par: recs.model_rows_source(*tables, users)),
        "popularity": dict(fit=lambda user, anime, rating, n_users, n_anime, par, device:
                           recs.popularity_scores(anime, n_anime, n_users).to(device),
                           source=lambda score, users, cols, par: score),
        "itemknn": dict(defaults=ITEMKNN_DEFAULTS, source=itemknn_source,
                        fit=lambda user, anime, rating, n_users, n_anime, par, device: recs.itemknn_fit(
                            user, anime, rating, n_users, n_anime, par["min_rating"], int(par["neighbours"]),
                            par["measure"], par["shrink"], par["min_support"], device=device)),
        "als": dict(defaults=ALS_DEFAULTS, fit=als_fit, source=lambda fit, users, cols, par: recs.als_rows_source(fit, users),
                    check=lambda par: ops.check_als(par["factors"], par["cg_steps"], par["reg"], par["alpha"])),
        "content": dict(defaults=dict(CONTENT_DEFAULTS, meta=None), check=content_check, fit=content_fit,
                        source=content_source)}


def _system_table():
    """``_systems()`` plus the systems of ``recs.EASE_SYSTEMS``: what every lookup by name goes through."""
    from . import ops, recs

    def ease_source(fit, users, cols, par):
        off, hist, _ = recs.history_csr(*cols[:3], users, min_rating=par["min_rating"])
        if int(par["neighbours"]):
            return recs.itemknn_rows_source(fit["knn"], off, hist)
        return recs.ease_rows_source(fit, off, hist)

    return dict(_systems(), ease=dict(
        defaults=EASE_DEFAULTS, check=lambda par: ops.check_ease(par["reg"], par["neighbours"]), source=ease_source,
        fit=lambda user, anime, rating, n_users, n_anime, par, device: recs.ease_fit(
            user, anime, rating, n_users, n_anime, par["min_rating"], par["reg"], int(par["neighbours"]), device=device)))


def _system_lookup():
    """``_system_table()`` plus the systems of ``recs.GRAPH_SYSTEMS``: what every lookup by name goes through."""
    from . import recs

    def rp3_source(fit, users, cols, par):
        off, hist, _ = recs.history_csr(*cols[:3], users, min_rating=par["min_rating"])
        return recs.rp3_rows_source(fit, off, hist)

    return dict(_system_table(), rp3=dict(
        defaults=RP3_DEFAULTS, check=lambda par: recs.check_rp3(par["alpha"], par["beta"], par["neighbours"]),
        source=rp3_source,
        fit=lambda user, anime, rating, n_users, n_anime, par, device: recs.rp3_fit(
            user, anime, rating, n_users, n_anime, par["min_rating"], par["alpha"], par["beta"], int(par["neighbours"]),
            device=device)))


def _system_layers():
    """``_system_lookup()`` plus the systems of ``recs.PAIRWISE_SYSTEMS``: what every lookup by name goes through."""
    from . import ops, recs

    def bpr_fit(user, anime, rating, n_users, n_anime, par, device):
        u, a, r = (recs._host(c) for c in (user, anime, rating))
        liked = r.astype(np.float32) >= np.float32(par["min_rating"])
        return recs.bpr_fit(u[liked], a[liked], n_users, n_anime, par["factors"], int(par["epochs"]), par["batch"],
                            par["lr"], par["reg"], par["tries"], par["bias"], seed=int(par["seed"]), device=device)

    def bpr_check(par):
        ops.check_bpr(par["factors"], par["batch"], par["tries"], par["lr"], par["reg"], par["bias"])
        if int(par["epochs"]) < 0:
            raise ValueError("bpr: epochs = %d must be >= 0" % int(par["epochs"]))

    return dict(_system_lookup(), bpr=dict(
        defaults=BPR_DEFAULTS, check=bpr_check, fit=bpr_fit,
        source=lambda fit, users, cols, par: recs.bpr_rows_source(fit, users)))


def _system_params(given, used):
    """{system: its defaults overridden by ``given[system]``}, the pre-GPU check made for each system of ``used``"""
    table = _system_layers()
    params = {name: _member_params(s["defaults"], given.get(name), name) for name, s in table.items() if "defaults" in s}
    for name in used:
        table[name].get("check", lambda par: None)(params.get(name))
    return params


def _system_source(name, tables, cols, params, users, device):
    """The row source of system ``name`` for ``users``, the system fitted from the training columns ``cols`` = (user,
    anime, rating, n_users, n_anime) on ``device``; ``tables`` = the model's (U, A, head) on the device."""
    s, par = _system_layers()[name], params.get(name)
    return s["source"](s["fit"](*cols, par, device) if "fit" in s else tables, users, cols, par)


def baseline_names(baseline):
    """``evaluate_frame``'s ``baseline`` as a tuple of distinct names in the order of BASELINES, FITTED_BASELINES,
    FUSED_BASELINES, TUNED_BASELINES, CONTENT_BASELINES, LINEAR_BASELINES, GRAPH_BASELINES, then PAIRWISE_BASELINES: None
    -> (), a name or a sequence of names; ValueError for anything else."""
    if baseline is None:
        return ()
    known = (BASELINES + FITTED_BASELINES + FUSED_BASELINES + TUNED_BASELINES + CONTENT_BASELINES + LINEAR_BASELINES +
             GRAPH_BASELINES + PAIRWISE_BASELINES)
    names = [baseline] if isinstance(baseline, str) else list(baseline)
    for b in names:
        if b not in known:
            raise ValueError("baseline %r is not supported (supported: %s, or None)" % (b, ", ".join(known)))
    return tuple(b for b in known if b in names)


def _ci_columns(columns, boot, system, others, key):
    """The bootstrap's columns of one system's figures: ``columns`` maps a column name to the bootstrap metric(s) behind it
    (a name, or a list of names for a frame column with one row per k).  Returns {column + "_lo" / "_hi": ...} and, for
    every system of ``others`` (name -> suffix), {column + "_diff_" + suffix (+ "_lo" / "_hi"), column + "_p_" + suffix},
    where ``key(column, part)`` places the part ("lo", "diff_x", ...) in the column's name."""
    out = {}

    def pick(cell, metric):
        return [cell[m] for m in metric] if isinstance(metric, list) else cell[metric]

    for col, metric in columns.items():
        fig = {m: boot["figures"][system][m] for m in (metric if isinstance(metric, list) else [metric])}
        for part in ("lo", "hi"):
            out[key(col, part)] = pick({m: f[part] for m, f in fig.items()}, metric)
        for other, suffix in others.items():
            d = boot["diffs"][other]
            for part, name in (("diff", "diff_" + suffix), ("lo", "diff_%s_lo" % suffix), ("hi", "diff_%s_hi" % suffix),
                               ("p", "p_" + suffix)):
                out[key(col, name)] = pick({m: d[m][part] for m in d}, metric)
    return out


def evaluate_frame(model, table, test_size, ks=(1, 5, 10, 50), min_rating=0.0, baseline=None, itemknn=None,
                   ci_replicates=0, ci_level=0.95, ci_seed=0, compare_model=None, als=None, hybrid=None,
                   hybrid_tune=None, content=None, ease=None, rp3=None, bpr=None):
    """How well a model ranks held-out ratings: each held-out (user, anime) rated at or above ``min_rating`` is ranked
    among the anime that user has no TRAINING rating for (the candidates model_recs would offer before the held-out
    rows were known), by predicted rating.  Returns (frame with one row per k: k, hit_rate, ndcg; summary dict:
    mrr, mean_rank, median_rank, n, n_users, test_size, min_rating and the frame's figures as hit_rate@k / ndcg@k).
    ``model``: weights_io.load_model's dict; its id tables must be the table's.
    ``baseline="popularity"``: the same targets under the same bits ranked by the number of training ratings of each
    anime instead (``recs.popularity_scores``, ``ops.score_rank``) — what recommending the most-rated unseen anime to
    everyone scores; the frame gains hit_rate_popularity / ndcg_popularity, the summary popularity_mrr,
    popularity_mean_rank, popularity_hit_rate@k and popularity_ndcg@k.
    ``baseline="itemknn"``: the same targets under the same bits ranked by an item-kNN fitted on the TRAINING slice alone
    (``recs.itemknn_fit``, ``recs.itemknn_rank``'s ranks), each listed user's history that user's training
    ratings at or above the threshold with weight 1; the same columns and keys under the name itemknn.  ``itemknn``: a
    dict overriding ITEMKNN_DEFAULTS (neighbours, measure, shrink, min_support, min_rating).
    ``baseline="als"``: the same targets under the same bits ranked by an implicit-feedback ALS factorisation fitted on
    the TRAINING slice alone (``recs.als_fit``, ``recs.als_rank``'s ranks), on the training pairs rated at or
    above its threshold, each with weight 1; the same columns and keys under the name als.  ``als``: a dict overriding
    ALS_DEFAULTS (factors, sweeps, cg_steps, alpha, reg, min_rating, seed) — the usual library defaults, not tuned on this
    data; a ``factors`` outside the supported widths is a ValueError before any GPU use.
    ``baseline="hybrid"``: the same targets under the same bits ranked by the fused score rows of several of the systems
    above (``recs.hybrid_rank``, ``ops.fuse_rows``), the item-kNN and ALS members fitted on the TRAINING
    slice with the ``itemknn`` / ``als`` parameters (one fit serves the baseline of the same name too); the same columns
    and keys under the name hybrid.  ``hybrid``: a dict overriding HYBRID_DEFAULTS (systems: names of
    ``recs.HYBRID_SYSTEMS``; weights: None = all 1; method: rrf or minmax; rrf_c) — the literature's defaults, not tuned
    on this data.
    ``baseline="hybrid_tuned"``: the hybrid's members, method and rrf_c with LEARNED weights: every
    target is ranked under every vector of ``recs.hybrid_weight_grid`` at once (``recs.hybrid_rank_grid``,
    ``ops.fuse_rank_grid``), the listed users are dealt into folds (``recs.hybrid_fold_deal``) and a user's targets take
    the ranks of the vector with the largest exact metric sum over the OTHER folds' users (``recs.hybrid_cross_fit``;
    ties to the lowest grid index, equal weights first), so no target helps choose the weights it is ranked with and the
    figures are free of selection leakage; the same columns and keys under the name hybrid_tuned, and the summary gains
    hybrid_tuned_metric, hybrid_tuned_grid (the number of vectors), hybrid_tuned_fold_weights (one vector per fold) and
    hybrid_tuned_weights (the best vector on ALL targets: what to pass to hybrid_recs, used for no reported figure).
    ``hybrid_tune``: a dict overriding HYBRID_TUNE_DEFAULTS (metric: ndcg@K, hit_rate@K or mrr; steps; folds >= 2; seed);
    an unknown metric, folds < 2 or a grid of more than 4095 vectors is a ValueError before any GPU use.
    ``baseline="content"``: the same targets under the same bits ranked by the content-based system:
    TF-IDF item vectors from the metadata (``recs.content_fit``: no rating takes part in them), each listed user's profile
    the weighted mean of the vectors of that user's TRAINING ratings at or above its threshold (``recs.content_rank``'s
    ranks); the same columns and keys under the name content, and ``content`` is a member the hybrids take too.
    ``content``: a dict overriding CONTENT_DEFAULTS (columns, weight: one of ``recs.CONTENT_WEIGHTS``, min_rating, min_df,
    max_df) plus ``meta``: the metadata frame by the table's anime index (``metadata_by_index(table.anime_ids, ...)``),
    without which asking for the system is a ValueError before any GPU use.
    ``baseline="ease"``: the same targets under the same bits ranked by EASE (Steck 2019), the closed-form
    linear item-item model fitted on the TRAINING pairs rated at or above its threshold (``recs.ease_fit``,
    ``recs.ease_rank``'s ranks), each listed user's history that user's such pairs with weight 1; the same columns and keys
    under the name ease, and ``ease`` is a member the hybrids take too.  ``ease``: a dict overriding EASE_DEFAULTS (reg:
    500, the paper's value for a data set of about this many users, not tuned on this data; min_rating; neighbours: K > 0
    keeps the K largest weights of every row only); a reg that is not finite or not > 0 is a ValueError before any GPU use.
    ``baseline="rp3"``: the same targets under the same bits ranked by RP3beta (Paudel et al. 2017), the
    three-step random walk with a popularity penalty fitted on the TRAINING pairs rated at or above its threshold
    (``recs.rp3_fit``, ``recs.rp3_rank``'s ranks), each listed user's history that user's such pairs with weight 1; the same
    columns and keys under the name rp3, and ``rp3`` is a member the hybrids take too.  ``rp3``: a dict overriding
    RP3_DEFAULTS (alpha: 1, beta: 0.3, neighbours: 100 — common values from the literature, not tuned on this data;
    neighbours = 0 keeps the dense matrix; min_rating); an alpha or beta that is negative or not finite is a ValueError
    before any GPU use.
    ``baseline="bpr"``: the same targets under the same bits ranked by a BPR matrix factorisation (Rendle et al. 2009;
    DESIGN.md 4.27), the learned model with a PAIRWISE objective, fitted on the TRAINING slice alone (``recs.bpr_fit``,
    ``recs.bpr_rank``'s ranks) on the training pairs rated at or above its threshold; the same columns and keys under the
    name bpr, and ``bpr`` is a member the hybrids take too.  ``bpr``: a dict overriding BPR_DEFAULTS (factors, epochs,
    batch, lr, reg, tries, bias, min_rating, seed) — the literature's and the ``implicit`` library's common values, not
    tuned on this data; a ``factors`` outside the supported widths is a ValueError before any GPU use.
    A sequence of names gives each, in the order popularity, itemknn, als, hybrid, hybrid_tuned, content, ease, rp3, bpr.
    None: none.
    ``compare_model``: a second model dict over the same id tables, ranked by a second ``ops.predict_rank`` on the same
    targets and bits and reported as the system ``compare`` (the baselines' columns and keys under that name).
    ``ci_replicates`` > 0: a Poisson bootstrap over the held-out USERS (``recs.bootstrap_metrics``), seeded
    by ``ci_seed``, the unit keys the user indices: the frame gains <col>_lo / <col>_hi (the ``ci_level`` percentile
    interval) for hit_rate, ndcg and every other system's columns and, for every other system s, hit_rate_diff_<s> (the
    model's figure minus s's, on the same weights), hit_rate_diff_<s>_lo / _hi and the two-sided hit_rate_p_<s>, the same
    for ndcg; the summary gains the same for mrr and mean_rank and ci_replicates, ci_level, ci_seed, ci_n_rep_used.
    median_rank is no sum and gets no interval.  With the defaults the frame and the summary are what they were, key for
    key.  ValueError before any GPU use for ci_replicates < 0 or a ci_level outside (0, 1)."""
    import torch
    from . import ops, recs, weights_io
    baselines = baseline_names(baseline)
    ci_replicates, ci_level = recs.check_bootstrap(ci_replicates, ci_level)
    hyb_par = _member_params(HYBRID_DEFAULTS, hybrid, "hybrid")
    tune_par = _member_params(HYBRID_TUNE_DEFAULTS, hybrid_tune, "hybrid_tune")
    members = ()
    if "hybrid" in baselines or "hybrid_tuned" in baselines:
        members, hyb_w, hyb_method, hyb_c = recs.check_hybrid(hyb_par["systems"], hyb_par["weights"], hyb_par["method"],
                                                              hyb_par["rrf_c"])
    if "hybrid_tuned" in baselines:
        tune_metric, _ = recs.hybrid_tune_metric(tune_par["metric"])
        tune_grid = recs.hybrid_weight_grid(len(members), tune_par["steps"])
        recs.hybrid_fold_deal(0, tune_par["folds"], tune_par["seed"])        # (the check of folds; dealt below)
        tune_pick, tune_best = [0] * int(tune_par["folds"]), 0
    fitted = [s for s in (recs.HYBRID_SYSTEMS + recs.CONTENT_SYSTEMS + recs.EASE_SYSTEMS + recs.GRAPH_SYSTEMS +
                          recs.PAIRWISE_SYSTEMS) if s in baselines or s in members]     # each once
    params = _system_params({"itemknn": itemknn, "als": als, "content": content, "ease": ease, "rp3": rp3, "bpr": bpr},
                            fitted)
    U, A = _tables_of(model, table)
    others = baselines + (("compare",) if compare_model is not None else ())
    if compare_model is not None:
        cU, cA = _tables_of(compare_model, table)
    ks = sorted({int(k) for k in ks})
    if not ks or ks[0] < 1:
        raise ValueError("eval_k must list at least one k >= 1 (got %r)" % (ks,))
    users, row, anime, train = recs.held_out_targets(table, test_size, min_rating)
    base_rank = {b: np.zeros(0, np.int32) for b in others}
    if len(row):
        tU, tA = torch.as_tensor(U).cuda(), torch.as_tensor(A).cuda()
        seen = recs.listed_seen_bits(table.user[train], table.anime[train], users, table.n_users, table.n_anime)
        rank, _ = ops.predict_rank(tU, tA, weights_io.model_head(model), users, row, anime, watched_bits=seen)
        if compare_model is not None:
            base_rank["compare"], _ = ops.predict_rank(torch.as_tensor(cU).cuda(), torch.as_tensor(cA).cuda(),
                                                       weights_io.model_head(compare_model), users, row, anime,
                                                       watched_bits=seen)
        cols = (table.user[train], table.anime[train], table.rating[train], table.n_users, table.n_anime)
        sources = {}
        for s in fitted:        # one fit serves the baseline of that name and the hybrid's member of that name
            sources[s] = _system_source(s, (tU, tA, weights_io.model_head(model)), cols, params, users, seen.device)
            if s == "popularity" and s in baselines:        # the shared vector has an entry point of its own
                base_rank[s] = ops.score_rank(sources[s], len(users), row, anime, watched_bits=seen)
            elif s in baselines:
                base_rank[s] = recs.rows_rank_batched(sources[s], len(users), seen, row, anime, what=s + "_rank")
        if "hybrid" in baselines:
            base_rank["hybrid"] = recs.hybrid_rank([sources[m] for m in members], seen, row, anime, hyb_w, hyb_method,
                                                   hyb_c)
        if "hybrid_tuned" in baselines:
            grid_rank = recs.hybrid_rank_grid([sources[m] for m in members], seen, row, anime, tune_grid, hyb_method,
                                              hyb_c)
            sums, tune_best = recs.hybrid_fit_weights(grid_rank, row, len(users), tune_metric, table.n_anime)
            tune_fold = recs.hybrid_fold_deal(len(users), tune_par["folds"], tune_par["seed"])
            tune_pick = recs.hybrid_cross_fit(sums, tune_fold, tune_par["folds"])
            pick = torch.as_tensor(np.asarray(tune_pick, np.int64)[tune_fold[np.asarray(row, np.int64)]],
                                   device=grid_rank.device)
            base_rank["hybrid_tuned"] = grid_rank[pick, torch.arange(len(row), device=grid_rank.device)]
    else:
        rank = np.zeros(0, np.int32)
    m = recs.ranking_metrics(rank, ks)
    frame = pd.DataFrame({"k": ks, "hit_rate": [m["hit_rate"][k] for k in ks], "ndcg": [m["ndcg"][k] for k in ks]})
    summary = {"n": m["n"], "n_users": int(len(users)), "test_size": int(test_size), "min_rating": float(min_rating),
               "mrr": m["mrr"], "mean_rank": m["mean_rank"], "median_rank": m["median_rank"]}
    for k in ks:
        summary["hit_rate@%d" % k] = m["hit_rate"][k]
        summary["ndcg@%d" % k] = m["ndcg"][k]
    for name in others:
        b = recs.ranking_metrics(base_rank[name], ks)
        frame["hit_rate_" + name] = [b["hit_rate"][k] for k in ks]
        frame["ndcg_" + name] = [b["ndcg"][k] for k in ks]
        summary[name + "_mrr"], summary[name + "_mean_rank"] = b["mrr"], b["mean_rank"]
        for k in ks:
            summary["%s_hit_rate@%d" % (name, k)] = b["hit_rate"][k]
            summary["%s_ndcg@%d" % (name, k)] = b["ndcg"][k]
    if "hybrid_tuned" in baselines:
        summary.update({"hybrid_tuned_metric": tune_metric, "hybrid_tuned_grid": int(len(tune_grid)),
                        "hybrid_tuned_fold_weights": [[float(w) for w in tune_grid[i]] for i in tune_pick],
                        "hybrid_tuned_weights": [float(w) for w in tune_grid[tune_best]]})
    if ci_replicates:
        systems = dict([("model", rank)] + [(name, base_rank[name]) for name in others])
        boot = recs.bootstrap_metrics(systems, row, len(users), ks, ci_replicates, ci_seed, ci_level, unit_key=users,
                                      n_rows=table.n_anime)
        per_k = {"hit_rate": ["hit_rate@%d" % k for k in ks], "ndcg": ["ndcg@%d" % k for k in ks]}
        once = {"mrr": "mrr", "mean_rank": "mean_rank"}
        for col, v in _ci_columns(per_k, boot, "model", {o: o for o in others}, lambda c, part: c + "_" + part).items():
            frame[col] = v
        summary.update(_ci_columns(once, boot, "model", {o: o for o in others}, lambda c, part: c + "_" + part))
        for name in others:
            for col, v in _ci_columns(per_k, boot, name, {}, lambda c, part: "%s_%s_%s" % (c, name, part)).items():
                frame[col] = v
            summary.update(_ci_columns(once, boot, name, {}, lambda c, part: "%s_%s_%s" % (name, c, part)))
        summary.update({"ci_replicates": ci_replicates, "ci_level": ci_level, "ci_seed": int(ci_seed),
                        "ci_n_rep_used": boot["n_rep_used"]})
    return frame, summary


LISTS_COLUMNS = ["diversity", "k", "pool", "hit_rate", "ndcg", "mrr", "mean_similarity", "mean_max_similarity",
                 "coverage", "gini", "novelty"]


def evaluate_lists_frame(model, table, test_size, min_rating, diversities, k=10, pool=100, ci_replicates=0,
                         ci_level=0.95, ci_seed=0):
    """What ``diverse_recs --diversity`` costs in hits and buys in spread: for each value d of
    ``diversities`` every user with a held-out rating at or above ``min_rating`` gets the list
    ``recs.diverse_topk(..., k, pool, d)`` under evaluate_frame's mask (the anime the user has a TRAINING rating for), and
    ``recs.list_quality`` scores all lists at once: the held-out anime's place in its user's list (hit_rate, ndcg, mrr)
    beside the lists' own figures (mean_similarity, mean_max_similarity, coverage, gini, and novelty against the training
    slice's rating counts).  The users, the targets and the mask are evaluate_frame's, so the d = 0 row's hit_rate and ndcg
    are its hit_rate@k and ndcg@k.  Returns (frame with one row per d and the columns LISTS_COLUMNS; summary dict with the
    keys ``lists_<column>@<d>``).  ValueError for id tables that are not the table's, a d outside [0, 1], k < 1 or
    pool < k, before any GPU use.
    ``ci_replicates`` > 0: evaluate_frame's bootstrap over the same users and keys, on the targets' slots in the lists
    (``recs.hit_positions``; gain tables of length k): hit_rate, ndcg and mrr of every row gain _lo / _hi and, against the
    FIRST listed diversity on the same weights, <col>_diff (first - this row), <col>_diff_lo / _hi and <col>_p (0, 0, 0
    and 1 on the first row itself); the summary gains them under the same keys and lists_ci_n_rep_used.  The five spread
    figures are no sums over targets and get nothing."""
    import torch
    from . import ops, recs, weights_io
    U, A = _tables_of(model, table)
    ci_replicates, ci_level = recs.check_bootstrap(ci_replicates, ci_level)
    ds = [float(d) for d in diversities]
    if not ds or not all(0.0 <= d <= 1.0 for d in ds):      # (a NaN fails both comparisons)
        raise ValueError("lists_diversity must list at least one diversity in [0, 1] (got %r)" % (list(diversities),))
    k, pool = int(k), int(pool)
    if k < 1:
        raise ValueError("lists_k must be >= 1 (got %d)" % k)
    if pool < k:
        raise ValueError("lists_pool = %d is smaller than lists_k = %d" % (pool, k))
    users, row, anime, train = recs.held_out_targets(table, test_size, min_rating)
    rows, slots = [], {}
    if len(row):
        tU, tA = torch.as_tensor(U).cuda(), torch.as_tensor(A).cuda()
        head = weights_io.model_head(model)
        seen = recs.listed_seen_bits(table.user[train], table.anime[train], users, table.n_users, table.n_anime)
        count = recs.popularity_scores(table.anime[train], table.n_anime, table.n_users)
        Wh = ops.rownorm(tA, device=tA.device)
        for i, d in enumerate(ds):
            idx, _, _ = recs.diverse_topk(tU, tA, head, users, k, pool, d, seen)
            rows.append(recs.list_quality(Wh, idx, k, row, anime, item_count=count, n_raters=table.n_users))
            if ci_replicates:
                slots[i] = torch.as_tensor(recs.hit_positions(idx[:, :k], row, anime), device=idx.device)
    else:
        rows = [dict.fromkeys(LISTS_COLUMNS[3:], float("nan")) for _ in ds]
        slots = {i: np.zeros(0, np.int64) for i in range(len(ds))}
    columns = list(LISTS_COLUMNS)
    summary = {"lists_%s@%g" % (c, d): q[c] for d, q in zip(ds, rows) for c in LISTS_COLUMNS[3:]}
    if ci_replicates:
        boot = recs.bootstrap_metrics(slots, row, len(users), [k], ci_replicates, ci_seed, ci_level, unit_key=users,
                                      n_rows=k)
        metric = {"hit_rate": "hit_rate@%d" % k, "ndcg": "ndcg@%d" % k, "mrr": "mrr"}
        for i, q in enumerate(rows):
            q.update(_ci_columns(metric, boot, i, {}, lambda c, part: c + "_" + part))
            for c, m in metric.items():
                dv = boot["diffs"][i][m] if i else {"diff": 0.0, "lo": 0.0, "hi": 0.0, "p": 1.0}
                q.update({c + "_diff": dv["diff"], c + "_diff_lo": dv["lo"], c + "_diff_hi": dv["hi"], c + "_p": dv["p"]})
        extra = [c + s for c in metric for s in ("_lo", "_hi", "_diff", "_diff_lo", "_diff_hi", "_p")]
        columns += extra
        summary.update({"lists_%s@%g" % (c, d): q[c] for d, q in zip(ds, rows) for c in extra})
        summary["lists_ci_n_rep_used"] = boot["n_rep_used"]
    frame = pd.DataFrame([dict({"diversity": d, "k": k, "pool": pool}, **{c: q[c] for c in columns[3:]})
                          for d, q in zip(ds, rows)], columns=columns)
    return frame, summary


# ----------------------------------------------------------------------------------------
# user_prefs / user_recs
# ----------------------------------------------------------------------------------------
MAX_CATEGORIES = 128     # anirec_fave_profile counts at most 128 categories per call
MAX_SIM_USERS = 63       # anirec_user_recs(_ex): k_sim <= 63
MAX_USER_RECS = 256      # anirec_user_recs(_ex): n_recs <= 256
FAVE_COLUMNS = ["eng_version", "Source", "Genres"]
USER_RECS_COLUMNS = ["anime_id", "Name", "n_user_prefs", "Source", "Genres", "Sypnopsis", "Episodes",
                     "Japanese name", "Studios", "Premiered", "Score", "Type"]


def load_user_anime_df(path):
    """get_anime_df of user_prefs.py:62-80 / user_recs.py:104-126: 'Unknown' -> NaN, ``eng_version`` is the
    anime's Name (get_anime_name), rows in file order (no sort, unlike similar_anime's loader)."""
    df = pd.read_csv(path)
    df = df.replace("Unknown", np.nan)
    df["anime_id"] = df["MAL_ID"]
    df["japanese_name"] = df["Japanese name"]
    first = df.drop_duplicates("anime_id").set_index("anime_id")["Name"]
    df["eng_version"] = first.reindex(df["anime_id"]).to_numpy()
    keep = ["anime_id", "eng_version", "Score", "Genres", "Episodes", "Premiered", "Studios", "japanese_name",
            "Name", "Type", "Source", "Rating", "Members"]
    return df[[c for c in keep if c in df.columns]]


def category_tokens(cell):
    """The tokens get_genres / get_sources (user_prefs.py:95-136) count for one Genres / Source cell:
    ``str`` cells only, ``split(',')``, each ``strip()``ped."""
    return [t.strip() for t in cell.split(",")] if isinstance(cell, str) else []


def _category_bits(rows, n_cat):
    """uint32 [len(rows), ceil(n_cat/32)]: bit c of row a set iff c is in rows[a]."""
    bits = np.zeros((len(rows), max(1, (n_cat + 31) // 32)), np.uint32)
    for a, cs in enumerate(rows):
        for c in cs:
            bits[a, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return bits


def category_table(meta, column):
    """(names, cat_bits) over the anime index: ``names`` the sorted distinct tokens of ``meta[column]``,
    cat_bits uint32 [n_anime, ceil(len(names)/32)] with bit c of row a set iff anime a carries names[c]."""
    cells = meta[column].tolist()
    names = sorted({t for cell in cells for t in category_tokens(cell)})
    if len(names) > MAX_CATEGORIES:
        raise ValueError("column %r holds %d distinct tokens; the favourite-profile kernel counts at most %d "
                         "categories (anirec_fave_profile)" % (column, len(names), MAX_CATEGORIES))
    index = {n: i for i, n in enumerate(names)}
    return names, _category_bits([[index[t] for t in category_tokens(cell)] for cell in cells], len(names))


def favourite_indices(fav_bits, u, n_anime):
    """Anime indices whose bit is set in row ``u`` of the favourite-bit matrix (a torch tensor)."""
    row = fav_bits[int(u)].cpu().numpy().view(np.uint32)
    bits = np.unpackbits(row.view(np.uint8), bitorder="little")[:int(n_anime)]
    return np.nonzero(bits)[0]


def fave_frame(fav_idx, anime_ids, anime_df):
    """fave_genres + fave_sources + get_fave_df (user_prefs.py:215-275): the anime_df rows whose id is a
    favourite, in anime_df order and with anime_df's index, columns eng_version, Source, Genres."""
    ids = np.asarray(anime_ids)[np.asarray(fav_idx, np.int64)]
    f = anime_df[anime_df["anime_id"].isin(ids)]
    return pd.DataFrame(f[FAVE_COLUMNS])


def favourite_profiles(fav_bits, meta, users):
    """Genre and Source histograms of the favourites of ``users`` (user indices): one ({genre: count},
    {source: count}) pair per user, keyed as get_genres / get_sources key them (only tokens that occur).
    One anirec_fave_profile call over both tables (Source tokens after the genre tokens) when they fit its
    128 categories together, one call per table otherwise."""
    from . import recs
    gcells, scells = meta["Genres"].tolist(), meta["Source"].tolist()
    gnames, gbits = category_table(meta, "Genres")
    snames, sbits = category_table(meta, "Source")
    ng, ns = len(gnames), len(snames)
    if ng + ns <= MAX_CATEGORIES:
        gi = {n: i for i, n in enumerate(gnames)}
        si = {n: ng + i for i, n in enumerate(snames)}
        rows = [[gi[t] for t in category_tokens(g)] + [si[t] for t in category_tokens(x)]
                for g, x in zip(gcells, scells)]
        tables = [(ng + ns, _category_bits(rows, ng + ns))]
    else:
        tables = [(ng, gbits), (ns, sbits)]
    counts = [recs.fave_profile(fav_bits, bits, n, users=users).cpu().numpy() if n else
              np.zeros((len(users), 0), np.int32) for n, bits in tables]
    allc = np.concatenate(counts, axis=1)
    return [({n: int(c) for n, c in zip(gnames, allc[r, :ng]) if c > 0},
             {n: int(c) for n, c in zip(snames, allc[r, ng:]) if c > 0}) for r in range(len(users))]


def rating_indices(df, user_ids, anime_ids):
    """The rating table as (user index, anime index, rating) by the model's id tables (not by a re-encoded,
    filtered frame: the reference's index mismatch); rows whose ids the tables lack are dropped."""
    ui = pd.Index(np.asarray(user_ids)).get_indexer(df["user_id"].to_numpy())
    ai = pd.Index(np.asarray(anime_ids)).get_indexer(df["anime_id"].to_numpy())
    ok = (ui >= 0) & (ai >= 0)
    return ui[ok].astype(np.int32), ai[ok].astype(np.int32), df["rating"].to_numpy(np.float64)[ok]


def favourite_bits(df, user_ids, anime_ids, percentile):
    """Favourite-bit rows of every user (rating >= np.percentile of the user's OWN ratings, over all of them)."""
    import torch
    from . import recs
    ui, ai, r = rating_indices(df, user_ids, anime_ids)
    dev = torch.device("cuda")
    fav, _ = recs.user_favourites(torch.from_numpy(ui).to(dev), torch.from_numpy(ai).to(dev),
                                  torch.from_numpy(r).to(dev), len(user_ids), len(anime_ids), float(percentile))
    return fav


def random_user(df, min_ratings=400):
    """get_random_user (user_prefs.py:195-209, user_recs.py:245-259): a random user of the >= 400-rating frame
    main_df_by_id keeps; every user when none has that many."""
    import random
    n = df["user_id"].value_counts(dropna=True)
    pool = n[n >= int(min_ratings)].index.tolist() or n.index.tolist()
    return int(random.choice(pool))


def user_index(user_ids, user_id):
    pos = np.nonzero(np.asarray(user_ids) == int(user_id))[0]
    if len(pos) == 0:
        raise ValueError("user id %r is not in the model's user table" % (user_id,))
    return int(pos[0])


def user_prefs_frame(fav_bits, user_ids, anime_ids, anime_df, user_id):
    """(fave_df, genre_freq, source_freq) of one user (user_prefs.py:215-275 and get_genres / get_sources):
    the favourites frame and the two word-cloud frequency dicts, from one anirec_fave_profile call."""
    u = user_index(user_ids, user_id)
    fave_df = fave_frame(favourite_indices(fav_bits, u, len(anime_ids)), anime_ids, anime_df)
    meta = metadata_by_index(anime_ids, anime_df)
    genre_freq, source_freq = favourite_profiles(fav_bits, meta, [u])[0]
    return fave_df, genre_freq, source_freq


def _bits_of(mask):
    n = len(mask)
    bits = np.zeros((n + 31) // 32, np.uint32)
    nz = np.nonzero(mask)[0]
    np.bitwise_or.at(bits, nz >> 5, np.uint32(1) << (nz & 31).astype(np.uint32))
    return bits


def check_user_recs_limits(n_sim, n_recs):
    if not 1 <= int(n_sim) <= MAX_SIM_USERS:
        raise ValueError("recs_n_sim_ID = %d: anirec_user_recs counts the favourites of 1 to %d similar users "
                         "(k_sim <= 63)" % (int(n_sim), MAX_SIM_USERS))
    if not 1 <= int(n_recs) <= MAX_USER_RECS:
        raise ValueError("user_num_recs = %d: anirec_user_recs returns 1 to %d anime per query (n_recs <= 256)"
                         % (int(n_recs), MAX_USER_RECS))


def user_recs_frame(fav_bits, user_ids, anime_ids, anime_df, syn_df, sim_user_ids, fave_df, n, genres=None):
    """similar_user_recs (user_recs.py:708-794): count how many of the similar users (ids, best first) hold each
    anime as a favourite, skip every anime whose eng_version is named in the query's favourites frame (:743,753),
    keep anime present in all_anime.csv, rank by (count desc, best similar-user rank asc, anime index asc), first n.
    ``genres`` (--ID_spec_genres): by_genre's order — the ranked matches of genre 1, then those of genre 2 not yet
    listed, then genre 3 — cut at n.  Returns the reference's 12-column frame."""
    from . import recs
    check_user_recs_limits(len(sim_user_ids), n)
    meta = metadata_by_index(anime_ids, anime_df, syn_df)
    names = set(fave_df["eng_version"].tolist())
    excl = _bits_of(meta["eng_version"].isin(names).to_numpy() & meta["has_meta"].to_numpy())
    keep = meta["has_meta"].to_numpy()
    uid = pd.Index(np.asarray(user_ids))
    sim = uid.get_indexer(np.asarray(sim_user_ids)).astype(np.int32)[None, :]        # unknown ids: -1 = empty
    masks = [keep]
    if genres is not None:
        check_genres(genres, anime_df)
        wanted = [g for g in clean(list(genres)) if g != "none"]
        masks = [keep & genre_mask(meta["Genres"], [g]) for g in wanted]
    order, counts = [], []
    for m in masks:
        a, c = recs.user_recs(fav_bits, len(anime_ids), None, sim, int(n), exclude=excl[None, :], keep=_bits_of(m))
        for ai, ci in zip(a.cpu().numpy()[0].tolist(), c.cpu().numpy()[0].tolist()):
            if ai >= 0 and ai not in order:
                order.append(ai)
                counts.append(ci)
    order, counts = order[:int(n)], counts[:int(n)]
    rows = meta.iloc[order]
    return pd.DataFrame({
        "anime_id": rows["anime_id"].to_numpy(), "Name": rows["Name"].to_numpy(),
        "n_user_prefs": np.asarray(counts, np.int64), "Source": rows["Source"].to_numpy(),
        "Genres": rows["Genres"].to_numpy(), "Sypnopsis": rows["Sypnopsis"].to_numpy(),
        "Episodes": rows["Episodes"].to_numpy(), "Japanese name": rows["japanese_name"].to_numpy(),
        "Studios": rows["Studios"].to_numpy(), "Premiered": rows["Premiered"].to_numpy(),
        "Score": rows["Score"].to_numpy(), "Type": rows["Type"].to_numpy()}, columns=USER_RECS_COLUMNS)


_CLOUD_NOTE = []


def word_cloud(freqs, fn, width, height, background, colormap):
    """genre_cloud / source_cloud (user_prefs.py:139-190): a word cloud of ``freqs`` written to ``fn``.  With the
    wordcloud package: the reference's WordCloud parameters.  Without it: a matplotlib PNG of width x height pixels
    showing the same words, sized by frequency (logged once).  Returns what show_cloud can display."""
    width, height = int(width), int(height)
    try:
        from wordcloud import WordCloud
    except ImportError:
        WordCloud = None
    if WordCloud is not None and freqs:
        cloud = WordCloud(width=width, height=height, prefer_horizontal=0.85, background_color=background,
                          contour_width=0.05, colormap=colormap).generate_from_frequencies(freqs)
        cloud.to_file(fn)
        return cloud
    if not _CLOUD_NOTE:
        logging.getLogger().info("wordcloud is not installed: the word clouds are drawn with matplotlib")
        _CLOUD_NOTE.append(True)
    from matplotlib import colormaps
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    fig = Figure(figsize=(width / 100.0, height / 100.0), dpi=100, facecolor=background)
    FigureCanvasAgg(fig)
    ax = fig.add_axes([0, 0, 1, 1])
    ax.set_axis_off()
    ax.set_facecolor(background)
    words = sorted(freqs.items(), key=lambda kv: (-kv[1], kv[0]))
    top = max(freqs.values()) if freqs else 1
    cols = max(1, int(np.ceil(np.sqrt(len(words))))) if words else 1
    rows = max(1, int(np.ceil(len(words) / cols))) if words else 1
    cmap = colormaps[colormap]
    for i, (w, f) in enumerate(words):
        x, y = (i % cols + 0.5) / cols, 1.0 - (i // cols + 0.5) / rows
        ax.text(x, y, w, ha="center", va="center", fontsize=6 + 18 * f / top, color=cmap(0.15 + 0.7 * f / top),
                transform=ax.transAxes)
    fig.savefig(fn, dpi=100, facecolor=background)
    return fig


def show_cloud(cloud, interval):
    """show_cloud (user_prefs.py:193-206): display for ``interval`` ms — only where the backend is interactive."""
    import matplotlib
    import matplotlib.pyplot as plt
    if matplotlib.get_backend().lower() in ("agg", "pdf", "ps", "svg", "cairo", "template") or \
            "inline" in matplotlib.get_backend().lower():
        return False
    fig = plt.figure(figsize=(8, 6))
    timer = fig.canvas.new_timer(interval=int(interval))
    timer.add_callback(plt.close)
    if hasattr(cloud, "to_array"):
        plt.imshow(cloud, interpolation="bilinear")
    else:
        cloud.canvas.draw()
        plt.imshow(np.asarray(cloud.canvas.buffer_rgba()), interpolation="bilinear")
    plt.axis("off")
    timer.start()
    plt.show()
    return True
