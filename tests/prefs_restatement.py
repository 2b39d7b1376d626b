"""TEST INFRASTRUCTURE — NumPy / pandas restatement of the favourite profiles and of similar_user_recs with an
explicit exclusion set and a keep mask.  Only tests/ may import this module.

Follows user_prefs.py:95-136 (get_genres / get_sources: ``str`` cells, ``split(',')``, ``strip()``, counted over the
favourites frame) and user_recs.py:708-794 (similar_user_recs: the similar users' favourites minus the anime named in
the query's favourites frame, counted, ranked; by_genre's regrouping when ID_spec_genres is set).  Ties among equal
counts are ordered as the build defines them: best (lowest) similar-user rank, then anime index.
"""
import numpy as np


def unpack(bits, n):
    """uint32 words [..., ceil(n/32)] -> bool [..., n]."""
    b = np.ascontiguousarray(bits).view(np.uint32)
    return np.unpackbits(b.view(np.uint8), axis=-1, bitorder="little")[..., :n].astype(bool)


def pack(mask):
    mask = np.asarray(mask, bool)
    n = mask.shape[-1]
    pad = np.zeros(mask.shape[:-1] + ((-n) % 32,), bool)
    return np.packbits(np.concatenate([mask, pad], axis=-1), axis=-1, bitorder="little").view(np.uint32)


def fave_profile(fav_bits, n_anime, cat_bits, n_cat, users=None):
    """counts[r][c] = #{a : bit a of fav_bits[users[r]] and bit c of cat_bits[a]} (int64)."""
    fav = unpack(fav_bits, n_anime)
    if users is not None:
        fav = fav[np.asarray(users, np.int64)]
    cat = unpack(cat_bits, n_cat)[:n_anime]
    return np.rint(fav.astype(np.float64) @ cat.astype(np.float64)).astype(np.int64)   # exact below 2^53


def token_counts(cells):
    """get_genres / get_sources over a column: {token.strip(): count}."""
    out = {}
    for cell in cells:
        if isinstance(cell, str):
            for t in cell.split(","):
                out[t.strip()] = out.get(t.strip(), 0) + 1
    return out


def user_recs(fav, query_excl, sims, n, keep=None):
    """fav: list of sets of anime indices; query_excl: set skipped; sims: similar users best first (-1 empty);
    keep: set of allowed anime or None.  Returns (anime order, counts)."""
    counts, best = {}, {}
    for j, s in enumerate(sims):
        if s < 0:
            continue
        for a in fav[s]:
            if a in query_excl or (keep is not None and a not in keep):
                continue
            counts[a] = counts.get(a, 0) + 1
            best.setdefault(a, j)
    order = sorted(counts, key=lambda a: (-counts[a], best[a], a))[:n]
    return order, [counts[a] for a in order]


def by_genre_groups(order, genres_of, wanted, n):
    """by_genre (user_recs.py:476-527) on a ranked list: the items matching wanted[0] in rank order, then those of
    wanted[1] not yet listed, then wanted[2]; cut at n.  ``genres_of(a)`` -> the lower-cased, space-free Genres text;
    ``wanted`` cleaned genre names.  Returns (items, group index of each)."""
    out, grp = [], []
    for gi, g in enumerate(w for w in wanted if w != "none"):
        for a in order:
            if g in genres_of(a) and a not in out:
                out.append(a)
                grp.append(gi)
    return out[:n], grp[:n]
