"""Favourites and user-based recommendations — host side of ``anirec_user_favourites`` / ``anirec_user_recs``
(the consumer of the similar-users top-k).

Reference: user_recs/user_recs.py:377-404 (``fave_genres``: favourites = ratings at or above the 80th
percentile of the user's own ratings), :708-760 (``similar_user_recs``: count the similar users'
favourites the query user has not favourited, rank by count), similar_users.py:203-256.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .ops import _bit_words, _call, _err_flag, _finish, _i32, _outputs, _workspace


def _aligned(t):
    """Contiguous and 16-byte aligned (the kernels read four rows per lane): a sliced view is copied."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def user_favourites(user_idx, anime_idx, rating, n_users, n_anime, percentile=80.0):
    """Returns (fav_bits int32 [n_users, ceil(n_anime/32)], threshold float64 [n_users]).
    Bit a of row u is set iff rating(u, a) >= np.percentile(ratings of u, percentile).  A user without ratings has
    threshold NaN and no bit; an empty table is that for every user, answered here without a library call."""
    if not torch.cuda.is_available():
        raise _lib.AnirecError("no GPU: the anime_recommendations_amd recs path needs an MI355X")
    dev = user_idx.device
    u = _aligned(user_idx.to(torch.int32))
    a = _aligned(anime_idx.to(torch.int32))
    r = _aligned(rating.to(torch.float64))
    n = int(u.numel())
    ww = (int(n_anime) + 31) // 32
    if n == 0:          # np.percentile of no rating: no threshold, no favourite (the entry point takes n >= 1)
        return (torch.zeros(int(n_users), ww, dtype=torch.int32, device=dev),
                torch.full((int(n_users),), float("nan"), dtype=torch.float64, device=dev))
    fav, thr = _outputs(dev, (torch.int32, int(n_users), ww), (torch.float64, int(n_users)))
    err = _err_flag(dev)
    ws = _workspace(None, dev, "anirec_fav_workspace_bytes", n, int(n_users))
    _call("anirec_user_favourites", u, a, r, n, int(n_users), int(n_anime), float(percentile), fav, thr, err, ws, ws.numel())
    return _finish((fav, thr), err, True, "user / anime index out of range")


def user_recs(fav_bits, n_anime, query_users, sim_users, n_recs, exclude=None, keep=None):
    """Per query user the ``n_recs`` anime its similar users favourited most often (own favourites skipped).
    ``sim_users``: [nq, k_sim] user indices, best first, -1 = empty.  Returns (anime int32 [nq, n_recs]
    (-1 padded), count int32 [nq, n_recs]).

    ``exclude`` ([nq, ceil(n_anime/32)] bit words) replaces the query user's own favourite row as the skipped set
    (``query_users`` is then not read); ``keep`` ([ceil(n_anime/32)] bit words) limits the candidates to its set bits
    (anirec_user_recs_ex).  With both None this is anirec_user_recs."""
    dev = fav_bits.device
    sim = _i32(sim_users, dev)
    nq, k_sim = int(sim.shape[0]), int(sim.shape[1])
    out_a, out_c = _outputs(dev, (torch.int32, nq, int(n_recs)), (torch.int32, nq, int(n_recs)))
    if exclude is None and keep is None:
        q = _i32(query_users, dev)
        assert q.numel() == nq
        _call("anirec_user_recs", fav_bits, int(fav_bits.shape[0]), int(n_anime), q, sim, nq, k_sim, int(n_recs), out_a, out_c)
        return out_a, out_c
    ww = (int(n_anime) + 31) // 32
    if exclude is None:         # a keep mask alone: the query users' own favourites are still skipped
        q = torch.as_tensor(query_users, device=dev).to(torch.long)
        exclude = fav_bits[q]
    ex = _bit_words(exclude, dev, (nq, ww), "exclude")
    kp = None if keep is None else _bit_words(keep, dev, (ww,), "keep")
    _call("anirec_user_recs_ex", fav_bits, int(fav_bits.shape[0]), int(n_anime), sim, nq, k_sim, ex, kp, int(n_recs), out_a,
          out_c)
    return out_a, out_c


def fave_profile(fav_bits, cat_bits, n_cat, users=None):
    """Favourite profiles: int32 [n_rows, n_cat], entry [r, c] = number of favourites of user ``users[r]`` (every
    user when None) whose category row (``cat_bits`` [n_anime, ceil(n_cat/32)] bit words) has bit c set.
    Raises ValueError on a user index out of range."""
    dev = fav_bits.device
    n_cat = int(n_cat)
    if not 1 <= n_cat <= 128:
        raise ValueError("n_cat = %d: the profile kernel counts 1 to 128 categories" % n_cat)
    n_users = int(fav_bits.shape[0])
    cw = (n_cat + 31) // 32
    n_anime = int(cat_bits.shape[0])
    cat = _bit_words(cat_bits, dev, (n_anime, cw), "cat_bits")
    if int(fav_bits.shape[1]) != (n_anime + 31) // 32:
        raise ValueError("fav_bits has %d words per row, cat_bits describes %d anime" % (int(fav_bits.shape[1]), n_anime))
    u = None if users is None else _i32(users, dev).view(-1)
    n_rows = n_users if u is None else int(u.numel())
    counts = torch.empty(n_rows, n_cat, dtype=torch.int32, device=dev)
    err = _err_flag(dev)
    _call("anirec_fave_profile", fav_bits.contiguous(), n_users, n_anime, u, n_rows, cat, n_cat, counts, err)
    return _finish(counts, err, True, "fave_profile: user index out of range")


def ranking_metrics(rank, ks):
    """Ranking metrics of held-out anime from their ranks (``ops.predict_rank``; 0 = ranked first), in float64 on the
    host: {"hit_rate": {k: mean(rank < k)}, "ndcg": {k: mean(1 / log2(rank + 2) if rank < k else 0)},
    "mrr": mean(1 / (rank + 1)), "mean_rank", "median_rank", "n"}.  One relevant anime per row, so the ideal DCG is 1
    and NDCG@k is the discounted gain itself.  An empty rank set gives NaN metrics and n = 0."""
    r = rank.detach().cpu().numpy() if isinstance(rank, torch.Tensor) else np.asarray(rank)
    r = r.reshape(-1).astype(np.float64)
    ks = [int(k) for k in ks]
    n = int(r.size)
    if n == 0:
        nan = float("nan")
        return {"hit_rate": {k: nan for k in ks}, "ndcg": {k: nan for k in ks}, "mrr": nan, "mean_rank": nan,
                "median_rank": nan, "n": 0}
    if (r < 0).any():
        raise ValueError("ranking_metrics: negative rank")
    gain = 1.0 / np.log2(r + 2.0)
    return {"hit_rate": {k: float(np.mean(r < k)) for k in ks},
            "ndcg": {k: float(np.mean(np.where(r < k, gain, 0.0))) for k in ks},
            "mrr": float(np.mean(1.0 / (r + 1.0))), "mean_rank": float(np.mean(r)), "median_rank": float(np.median(r)),
            "n": n}


def _host(col):
    return col.detach().cpu().numpy() if isinstance(col, torch.Tensor) else np.asarray(col)


def held_out_targets(table, test_size, min_rating):
    """The ranking targets of a rating table: (users, target_row, target_anime, train) — the held-out rows of
    ``table.split(test_size)`` (the rows trainer.fit validates on) rated at or above ``min_rating``, as the sorted
    distinct user indices among them, each target's position in that list and its anime index; ``train`` is the
    training slice."""
    train, test = table.split(test_size)
    take = _host(table.rating[test]).astype(np.float64) >= float(min_rating)
    tu, ta = _host(table.user[test])[take], _host(table.anime[test])[take]
    users, row = np.unique(tu, return_inverse=True)
    return users.astype(np.int64), row.astype(np.int64).reshape(-1), ta.astype(np.int64), train


def listed_seen_bits(user_idx, anime_idx, users, n_users, n_anime, device="cuda:0"):
    """``ops.seen_bits`` of the listed users alone: int32 [len(users), ceil(n_anime/32)], row i the watched bits of
    user ``users[i]`` (distinct indices) in the rating list — the rows ``ops.seen_bits(...)[users]`` would hold, without
    the whole [n_users, words] table (769 MB at 350 000 users x 17 560 anime; 22 MB for 10 000 listed users).  The
    ratings' users are mapped to positions in the list through a lookup tensor and those of no listed user dropped."""
    from . import ops
    dev = user_idx.device if isinstance(user_idx, torch.Tensor) and user_idx.is_cuda else torch.device(device)
    u = torch.as_tensor(_host(user_idx) if not isinstance(user_idx, torch.Tensor) else user_idx, device=dev).long()
    a = torch.as_tensor(_host(anime_idx) if not isinstance(anime_idx, torch.Tensor) else anime_idx, device=dev)
    us = torch.as_tensor(np.asarray(users, np.int64), device=dev)
    if us.numel() and (int(us.min()) < 0 or int(us.max()) >= int(n_users)):
        raise ValueError("listed_seen_bits: listed user out of range")
    if u.numel() and (int(u.min()) < 0 or int(u.max()) >= int(n_users)):
        raise ValueError("listed_seen_bits: user index out of range")
    lut = torch.full((int(n_users),), -1, dtype=torch.int32, device=dev)
    lut[us] = torch.arange(int(us.numel()), dtype=torch.int32, device=dev)
    pos = lut[u]
    keep = pos >= 0
    return ops.seen_bits(pos[keep], a[keep].to(torch.int32), int(us.numel()), n_anime, device=dev)


def rank_figures(m, specs):
    """``ranking_metrics``' dict read through ranking specs (``schedule.split_rank_metrics``): {key: figure} in the
    specs' order, key ``hit_rate@K`` / ``ndcg@K`` / ``mrr``."""
    return {key: (m["mrr"] if kind == "mrr" else m[kind][k]) for key, kind, k in specs}


def popularity_scores(anime_idx, n_anime, n_users=None):
    """The popularity baseline's score vector: fp32 [n_anime], the number of ratings each anime has in ``anime_idx``
    (a slice of a rating table's anime column, NumPy or torch; the result lives where a torch input does, else on the
    host) — the ``score`` of ``ops.score_rank``.  A count is exact in fp32 below 2**24, and an anime has at most one
    rating per user (preprocess drops duplicate pairs): ValueError for ``n_users >= 2**24`` and, whatever ``n_users``
    says, for a count that reaches 2**24."""
    n_anime = int(n_anime)
    if n_anime < 1:
        raise ValueError("popularity_scores: n_anime must be >= 1")
    if n_users is not None and int(n_users) >= 1 << 24:
        raise ValueError("popularity_scores: n_users >= 2**24 (%d): rating counts that large are not exact in fp32"
                         % int(n_users))
    a = anime_idx if isinstance(anime_idx, torch.Tensor) else torch.as_tensor(np.asarray(anime_idx))
    a = a.reshape(-1).to(torch.int64)
    if a.numel() and bool(((a < 0) | (a >= n_anime)).any()):
        raise ValueError("popularity_scores: anime index out of range")
    counts = torch.bincount(a, minlength=n_anime)
    if int(counts.max()) >= 1 << 24:
        raise ValueError("popularity_scores: an anime has 2**24 ratings or more: not exact in fp32")
    return counts.to(torch.float32)


def _pool_topk(fn, what, weight, U, A, head, users, k, pool, watched_bits, check, rerank):
    """The skeleton of ``diverse_topk`` and ``calibrated_topk`` (``fn``; ``what`` names its ``weight``): the range
    checks, weight 0 as ``ops.predict_topk(..., k)`` itself, ``pool`` clamped to the number of anime, ``check(pool, k,
    weight)`` before any GPU work (k <= pool <= the kernel's list limit), the ``pool`` best by predicted rating, and
    ``rerank(cand, p, k, weight)`` -> (idx, pool slot, rating, penalty).  Returns (idx, rating, penalty or None)."""
    from . import ops
    k, pool, weight = int(k), int(pool), float(weight)
    if not 0.0 <= weight <= 1.0:
        raise ValueError("%s: %s = %r must be in [0, 1]" % (fn, what, weight))
    if k < 1:
        raise ValueError("%s: k must be >= 1" % fn)
    if pool < k:
        raise ValueError("%s: pool = %d is smaller than k = %d" % (fn, pool, k))
    if weight == 0.0:
        return ops.predict_topk(U, A, head, users, k, watched_bits) + (None,)
    pool = min(pool, int(A.shape[0]))
    check(pool, k, weight)
    cand, p = ops.predict_topk(U, A, head, users, pool, watched_bits)
    idx, _, score, pen = rerank(cand, p, k, weight)
    return idx, score, pen


def diverse_topk(U, A, head, users, k, pool, diversity, watched_bits=None):
    """Diversified top-k per user: the ``pool`` best unwatched anime by predicted rating
    (``ops.predict_topk``), re-ranked greedily by ``ops.mmr_rerank`` on the normalised anime rows with
    ``lam = 1 - diversity`` — each pick trades a candidate's rating against its largest cosine to an anime already
    picked.  Batched over ``users`` (rows of ``U``, which may be folded rows); ``watched_bits`` as predict_topk.
    ``pool`` is clamped to the number of anime.  ``diversity`` == 0 is ``ops.predict_topk(..., k)`` itself: no pool,
    no re-rank, the bits of model_recs.
    Returns (idx int32 [n_users, k], p fp32 [n_users, k], pen fp32 [n_users, k] or None at diversity 0): the anime, their
    predicted ratings and each pick's largest cosine to the picks before it (0 for the first); -1 / NaN / NaN padded.
    Raises ValueError for ``diversity`` outside [0, 1], k < 1, pool < k, and, at diversity > 0, for k above the number of
    anime or a pool above anirec_mmr_max_cand(width)."""
    from . import ops
    return _pool_topk("diverse_topk", "diversity", diversity, U, A, head, users, k, pool, watched_bits,
                      lambda pool, k, w: ops.check_mmr(A.shape[1], pool, k, 1.0 - w),
                      lambda cand, p, k, w: ops.mmr_rerank(ops.rownorm(A, device=A.device), cand, p, k, 1.0 - w))


def calibrated_topk(U, A, head, users, k, pool, calibration, cat_bits, n_cat, profile, watched_bits=None):
    """Calibrated top-k per user: the ``pool`` best unwatched anime by predicted rating
    (``ops.predict_topk``), re-ranked greedily by ``ops.calibrate_rerank`` — each pick trades a candidate's rating
    against the distance between the list's category proportions and the user's own (``profile``: one row of
    ``fave_profile(..., users=users)`` counts per entry of ``users``; ``cat_bits`` [n_anime, ceil(n_cat/32)]: the
    category bit rows of the anime).  Batched over ``users``; ``watched_bits`` as predict_topk.  ``pool`` is clamped to
    the number of anime.  ``calibration`` == 0 is ``ops.predict_topk(..., k)`` itself: no pool, no re-rank, the bits of
    model_recs.
    Returns (idx int32 [n_users, k], p fp32 [n_users, k], miscal fp32 [n_users, k] or None at calibration 0): the anime,
    their predicted ratings and the miscalibration of the list down to and including each pick; -1 / NaN / NaN padded.
    Raises ValueError for ``calibration`` outside [0, 1], k < 1, pool < k, and, at calibration > 0, for k above the
    number of anime, a pool above anirec_calibrate_max_cand() or ``n_cat`` outside 1 .. 128."""
    from . import ops
    return _pool_topk("calibrated_topk", "calibration", calibration, U, A, head, users, k, pool, watched_bits,
                      lambda pool, k, w: ops.check_calibrate(n_cat, pool, k, w),
                      lambda cand, p, k, w: ops.calibrate_rerank(cat_bits, n_cat, cand, p, profile, k, w))


def list_calibration(lists, cat_bits, n_cat, profile):
    """The miscalibration of lists (``ops.list_calibration``): (miscal fp32 [n_lists], num int64, den int64) on the
    device — the total variation distance between the category-token distribution of ``lists[l]`` (rows of ``cat_bits``,
    -1 padded) and that of ``profile[l]``, miscal = float32(num / den)."""
    from . import ops
    return ops.list_calibration(cat_bits, n_cat, lists, profile)


def group_csr(groups, user_ids):
    """The CSR ``ops.group_topk`` takes, from groups given as lists of user ids: (users int64 [n_distinct]: the rows of
    ``user_ids`` (the model's index -> id table) of the distinct members, in order of first appearance, each once;
    offsets int64 [n_groups + 1]; member_row int32 [n_members]: each member's position in ``users``, group after
    group in the order given, a repeated id repeated).  A user may be in any number of groups.  ValueError, naming
    them, for ids without a row."""
    sizes = [len(g) for g in groups]
    flat = np.asarray([int(u) for g in groups for u in g], np.int64)
    offsets = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    table = np.asarray(user_ids, np.int64)
    distinct, first, inverse = np.unique(flat, return_index=True, return_inverse=True)
    by_first = np.argsort(first, kind="stable")             # distinct ids in order of first appearance
    place = np.empty(len(distinct), np.int64)
    place[by_first] = np.arange(len(distinct))
    ids = distinct[by_first]
    order = np.argsort(table, kind="stable")
    pos = np.searchsorted(table[order], ids)
    pos[pos == len(table)] = 0
    has = (table[order][pos] == ids) if len(table) else np.zeros(len(ids), bool)
    if not bool(has.all()):
        raise ValueError("group_csr: user id(s) %s have no embedding row" % ", ".join(str(int(x)) for x in ids[~has][:20]))
    return order[pos].astype(np.int64), offsets, place[inverse.reshape(-1)].astype(np.int32)


def group_topk(model_or_tables, groups, k, mode="mean", floor=None, watched_bits=None, exclude_bits=None,
               member_ratings=False, device="cuda:0"):
    """A top-k list per group of user ids: ``group_csr`` of ``groups``, then ``ops.group_topk``.
    ``model_or_tables``: ``weights_io.load_model``'s dict (with its id tables), or (U, A, head, user_ids) with the
    tables as arrays or device tensors.  ``watched_bits``: None, or a callable given ``users`` (the rows of the distinct
    members) that returns their [len(users), ceil(n_anime/32)] bit rows (``listed_seen_bits`` with the rating list bound
    is one).  ``exclude_bits`` [n_groups, ceil(n_anime/32)], ``mode``, ``floor``, ``member_ratings``: as ops.group_topk.
    Returns (idx, score[, member_p], csr) with csr = (users, offsets, member_row)."""
    from . import ops, weights_io
    if isinstance(model_or_tables, dict):
        model = model_or_tables
        if model.get("user_ids") is None:
            raise ValueError("group_topk: the model file has no id tables")
        U, A, head, user_ids = model["U"], model["A"], weights_io.model_head(model), model["user_ids"]
    else:
        U, A, head, user_ids = model_or_tables
    csr = group_csr(groups, user_ids)
    tU = U if isinstance(U, torch.Tensor) and U.is_cuda else torch.as_tensor(np.ascontiguousarray(U, np.float32), device=device)
    tA = A if isinstance(A, torch.Tensor) and A.is_cuda else torch.as_tensor(np.ascontiguousarray(A, np.float32), device=device)
    wb = watched_bits(csr[0]) if callable(watched_bits) else watched_bits
    out = ops.group_topk(tU, tA, head, csr[0], csr[1], csr[2], k, mode=mode, floor=floor, watched_bits=wb,
                         exclude_bits=exclude_bits, member_ratings=member_ratings)
    return out + (csr,)


def gini(counts):
    """Gini coefficient of non-negative counts, float64 on the host: with the n counts sorted ascending,
    sum_i (2 i - n - 1) c_i / (n sum c), i 1-based — 0 for equal counts, (n - 1) / n when one holds everything.  NaN for
    no counts or an all-zero vector."""
    c = np.sort(np.asarray(counts, np.float64).reshape(-1))
    n, total = c.size, float(c.sum()) if c.size else 0.0
    if n == 0 or total == 0.0:
        return float("nan")
    return float(((2.0 * np.arange(1, n + 1) - n - 1.0) * c).sum() / (n * total))


def hit_positions(lists, target_row, target_anime):
    """Where each target is in its list: int64 [n_t] on the host, the lowest slot of ``lists[target_row[t]]`` that holds
    ``target_anime[t]``, -1 where none does.  ``lists``: an int [n_lists, k] tensor; the compare runs where it lives."""
    dev = lists.device
    tr = torch.as_tensor(np.asarray(_host(target_row), np.int64), device=dev).reshape(-1)
    ta = torch.as_tensor(np.asarray(_host(target_anime), np.int64), device=dev).reshape(-1)
    if tr.shape != ta.shape:
        raise ValueError("hit_positions: target_row and target_anime must have one length")
    if tr.numel() == 0:
        return np.zeros(0, np.int64)
    if int(tr.min()) < 0 or int(tr.max()) >= int(lists.shape[0]):
        raise ValueError("hit_positions: target_row out of range")
    if int(ta.min()) < 0:
        raise ValueError("hit_positions: target_anime out of range")
    k = int(lists.shape[1])
    pos = torch.full((tr.numel(),), -1, dtype=torch.int64, device=dev)
    for t0 in range(0, int(tr.numel()), 1 << 22):             # (bounds the [n_t, k] compare)
        t = slice(t0, t0 + (1 << 22))
        hit = lists[tr[t]].to(torch.int64) == ta[t].unsqueeze(1)
        slot = torch.where(hit, torch.arange(k, device=dev).expand_as(hit), torch.full_like(hit, k, dtype=torch.int64))
        first = slot.min(dim=1).values
        pos[t] = torch.where(first < k, first, torch.full_like(first, -1))
    return pos.cpu().numpy()


LIST_FIGURES = ("mean_similarity", "mean_max_similarity", "coverage", "gini", "novelty")
HIT_FIGURES = ("hit_rate", "ndcg", "mrr")


def list_figures(idx, n_rows, sim_max, sim_sum, target_row=None, target_anime=None, item_count=None, n_raters=None):
    """``list_quality``'s figures from lists and their similarity structure, wherever the tensors live (no kernel):
    ``idx`` int [n_lists, k] (-1 = an empty slot), ``sim_max`` / ``sim_sum`` fp32 [n_lists, k] as
    ``ops.list_similarity`` writes them, ``n_rows`` the rows of the table the lists index."""
    if (target_row is None) != (target_anime is None):
        raise ValueError("list_quality: target_row and target_anime come together")
    if item_count is not None and n_raters is None:
        raise ValueError("list_quality: item_count needs n_raters")
    n_rows, n_lists = int(n_rows), int(idx.shape[0])
    nan = float("nan")
    out = {"n_lists": n_lists, "mean_similarity": nan, "mean_max_similarity": nan, "coverage": nan, "gini": nan}
    if item_count is not None:
        out["novelty"] = nan
    if target_row is not None:
        out.update({"n_targets": int(np.asarray(_host(target_row)).size), "hit_rate": nan, "ndcg": nan, "mrr": nan})
    if n_lists == 0:
        if out.get("n_targets"):
            raise ValueError("hit_positions: target_row out of range")
        return out
    present = idx >= 0
    p = present.sum(dim=1).to(torch.float64)
    pairs = p >= 2
    if bool(pairs.any()):
        zero = torch.zeros((), dtype=torch.float64, device=idx.device)
        tot_sum = torch.where(present, sim_sum.to(torch.float64), zero).sum(dim=1)[pairs]
        tot_max = torch.where(present, sim_max.to(torch.float64), zero).sum(dim=1)[pairs]    # (the first one's is 0)
        pp = p[pairs]
        out["mean_similarity"] = float((tot_sum / (pp * (pp - 1.0) / 2.0)).mean())
        out["mean_max_similarity"] = float((tot_max / (pp - 1.0)).mean())
    listed = idx[present].to(torch.int64)
    exposure = torch.bincount(listed, minlength=n_rows)
    out["coverage"] = float(int((exposure > 0).sum())) / n_rows
    out["gini"] = gini(exposure.cpu().numpy())
    if item_count is not None:
        cnt = torch.as_tensor(_host(item_count) if not isinstance(item_count, torch.Tensor) else item_count,
                              device=idx.device).to(torch.float64).reshape(-1)
        if cnt.numel() != n_rows:
            raise ValueError("list_quality: item_count must hold one count per row of What")
        if listed.numel():
            out["novelty"] = float((-torch.log2((cnt[listed] + 1.0) / (float(n_raters) + 1.0))).mean())
    if target_row is not None:
        pos = hit_positions(idx, target_row, target_anime)
        if pos.size:
            found = pos >= 0
            r = np.where(found, pos, 0).astype(np.float64)
            out["hit_rate"] = float(np.mean(found))
            out["ndcg"] = float(np.mean(np.where(found, 1.0 / np.log2(r + 2.0), 0.0)))
            out["mrr"] = float(np.mean(np.where(found, 1.0 / (r + 1.0), 0.0)))
    return out


def list_quality(What, lists, k=None, target_row=None, target_anime=None, item_count=None, n_raters=None):
    """Figures of many top-k lists at once, over the first ``k`` columns of ``lists`` (all of them when
    None): int [n_lists, K] rows of the normalised table ``What`` (``ops.rownorm`` output, on the device), -1 = an empty
    slot, as ``ops.predict_topk`` / ``diverse_topk`` write them.  Every figure is float64; p = a list's present slots.
        mean_similarity      mean over the lists with p >= 2 of (sum of ``ops.list_similarity``'s sim_sum) / (p (p - 1) / 2):
                             the list's mean pairwise cosine
        mean_max_similarity  mean over the same lists of the mean of sim_max over the present slots after the first
        coverage             distinct listed rows / n_rows
        gini                 ``gini`` of the rows' exposure counts over all n_rows (NaN when nothing is listed)
        novelty              mean over the present slots of -log2((item_count[a] + 1) / (n_raters + 1)); with
                             ``item_count`` ([n_rows] rating counts, ``popularity_scores``) and ``n_raters`` only
        hit_rate, ndcg, mrr  with targets (``target_row[t]``: a list, ``target_anime[t]``: a row of What): pos = the
                             target's lowest slot in its list; mean of [found], of 1 / log2(pos + 2) and of 1 / (pos + 1),
                             0 where it is not found
        n_lists, n_targets
    An empty input gives NaN.  Only the similarities run a kernel (``ops.list_similarity``); exposure, novelty and hit
    positions are plain torch (``list_figures``)."""
    from . import ops
    if lists.dim() != 2:
        raise ValueError("list_quality: lists must be [n_lists, k]")
    k = int(lists.shape[1]) if k is None else int(k)
    if not 1 <= k <= int(lists.shape[1]):
        raise ValueError("list_quality: k = %d must be in 1 .. %d (the columns of lists)" % (k, int(lists.shape[1])))
    ops.check_list_similarity(What.shape[1], k)
    idx = lists[:, :k].to(device=What.device, dtype=torch.int32).contiguous()
    sims = ops.list_similarity(What, idx) if idx.shape[0] else (None, None)
    return list_figures(idx, What.shape[0], sims[0], sims[1], target_row, target_anime, item_count, n_raters)


EXPLAIN_WEIGHTS = ("rating", "similarity")


def history_csr(user_idx, anime_idx, rating, users, min_rating=0.0):
    """The CSR ``explain_topk`` takes, from a rating table's training columns (``user_idx``, ``anime_idx``: dense
    indices; ``rating``: the scaled target the trainer uses; NumPy or torch): list i is the ratings of user
    ``users[i]`` (a repeated user gets the history again) in their order in the table, those below ``min_rating``
    (compared in fp32) or NaN dropped.  A user without ratings has an empty history.
    Returns (offsets int64 [len(users) + 1], hist_idx int32 [n], hist_rating fp32 [n]) on the host."""
    u = _host(user_idx).reshape(-1).astype(np.int64)
    a = _host(anime_idx).reshape(-1)
    r = _host(rating).reshape(-1).astype(np.float32)
    if not len(u) == len(a) == len(r):
        raise ValueError("history_csr: user_idx, anime_idx and rating must have one entry per rating")
    users = np.asarray(users, np.int64).reshape(-1)
    keep = r >= np.float32(min_rating)
    u, a, r = u[keep], a[keep], r[keep]
    order = np.argsort(u, kind="stable")                    # by user, the table's order within a user
    su = u[order]
    lo, hi = np.searchsorted(su, users, "left"), np.searchsorted(su, users, "right")
    offsets = np.zeros(len(users) + 1, np.int64)
    np.cumsum(hi - lo, out=offsets[1:])
    take = order[np.repeat(lo - offsets[:-1], hi - lo) + np.arange(int(offsets[-1]))]
    return offsets, a[take].astype(np.int32), r[take]


def explain_topk(What_or_A, lists, offsets, hist_idx, hist_rating, m=3, weight="rating", normalised=None, device="cuda:0"):
    """Why each anime of many lists is there (``ops.explain_lists``): for every listed anime the ``m``
    entries of the list's own history with the largest ``weight * cosine``.  ``lists``: int [n_lists, k] rows of the
    anime table, -1 = an empty slot — ``ops.predict_topk``'s, ``diverse_topk``'s, ``group_topk``'s (with the members'
    histories concatenated) or a folded user's (with the fold-in CSR); list l's history is
    ``hist_idx[offsets[l]:offsets[l+1]]`` with the scaled ratings ``hist_rating`` (``history_csr``).
    ``weight``: ``rating`` weights an entry by its rating, ``similarity`` by 1 (the nearest history rows).
    ``What_or_A``: a device tensor is taken as the normalised table (``ops.rownorm`` output) as it is, a host array as
    the anime table A and normalised here; ``normalised`` = True / False says which instead.
    Returns (pos int32, sim fp32, contrib fp32, hist_row int32), each [n_lists, k, m] on the device: ``ops.explain_lists``'
    three tensors and the anime row at each pos (``hist_idx[offsets[l] + pos]``), -1 where there is no pick."""
    from . import ops
    w = str(weight).strip().lower()
    if w not in EXPLAIN_WEIGHTS:
        raise ValueError("explain_topk: weight %r is not one of %s" % (weight, ", ".join(EXPLAIN_WEIGHTS)))
    on_dev = isinstance(What_or_A, torch.Tensor) and What_or_A.is_cuda
    if normalised is None:
        normalised = on_dev
    T = What_or_A if on_dev else torch.as_tensor(np.ascontiguousarray(_host(What_or_A), np.float32), device=device)
    What = T if normalised else ops.rownorm(T, device=T.device)
    dev = What.device
    li = torch.as_tensor(lists, device=dev).to(torch.int32)
    if li.dim() != 2:
        raise ValueError("explain_topk: lists must be [n_lists, k]")
    ops.check_explain(What.shape[1], li.shape[1], m)
    off = torch.as_tensor(offsets).to(torch.int64).cpu()
    hi = torch.as_tensor(hist_idx, device=dev).to(torch.int32).reshape(-1)
    hw = torch.as_tensor(hist_rating, device=dev).to(torch.float32).reshape(-1)
    if w == "similarity":
        hw = torch.ones_like(hw)
    pos, sim, contrib = ops.explain_lists(What, li, off, hi, hw, m)
    if hi.numel() == 0:
        return pos, sim, contrib, torch.full_like(pos, -1)
    at = (off[:-1].to(dev).view(-1, 1, 1) + pos.clamp(min=0).long()).clamp(max=hi.numel() - 1)
    hist_row = torch.where(pos >= 0, hi[at], torch.full_like(pos, -1))
    return pos, sim, contrib, hist_row


def _unit_rows(What_or_table, normalised, device):
    """A table as ``explain_topk`` takes it: a device tensor is the normalised table as it is, a host array the raw
    table, normalised here; ``normalised`` = True / False says which instead."""
    from . import ops
    on_dev = isinstance(What_or_table, torch.Tensor) and What_or_table.is_cuda
    if normalised is None:
        normalised = on_dev
    T = What_or_table if on_dev else torch.as_tensor(np.ascontiguousarray(_host(What_or_table), np.float32), device=device)
    if T.dim() != 2:
        raise ValueError("a table must be [n_rows, width]")
    return T if normalised else ops.rownorm(T, device=T.device)


def usable_rows(What):
    """bool [n_rows] on the device: the rows anirec_kmeans_assign takes (every element finite and at most 2 in
    magnitude; a zero row normalised to NaN is not one)."""
    return (What.abs() <= 2).all(dim=1)


def cluster_rows(What_or_table, k, seed=0, max_iter=50, init=None, normalised=None, device="cuda:0"):
    """Spherical k-means on an embedding table (``ops.kmeans_fit``): ``k`` clusters of the unit rows by
    cosine.  ``What_or_table``: a device tensor is taken as the normalised table (``ops.rownorm`` output) as it is, a
    host array as the raw table and normalised here; ``normalised`` = True / False says which instead.
    ``init``: None draws k distinct usable rows with ``np.random.default_rng(seed).choice`` (sorted row order kept as
    drawn) as the first centroids; an int array [k] names the rows; a float array [k, width] is the centroids themselves.
    Returns a dict: C fp32 [k, width], assign int32 [n_rows] (-1 for a row that is not usable), sim fp32 [n_rows],
    count int32 [k] (device tensors), iters, converged, init_rows (the drawn or given rows as a NumPy array, else None).
    Raises ValueError for k outside 1 .. KMEANS_MAX_K, fewer usable rows than k, or an ``init`` of another shape."""
    from . import ops
    shape = tuple(What_or_table.shape)
    if len(shape) != 2:
        raise ValueError("cluster_rows: a table must be [n_rows, width]")
    # the refusals that need no device come first
    dim, k, max_iter = ops.check_kmeans(shape[1], k, max_iter)
    if k > shape[0]:
        raise ValueError("cluster_rows: k = %d clusters but the table has only %d usable rows" % (k, shape[0]))
    init_rows = arr = None
    if init is not None:
        arr = np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init)
        if arr.ndim == 1 and arr.shape[0] == k and np.issubdtype(arr.dtype, np.integer):
            if arr.min() < 0 or arr.max() >= shape[0]:
                raise ValueError("cluster_rows: init row out of range")
            init_rows = arr.astype(np.int64)
        elif arr.shape != (k, dim) or not np.issubdtype(arr.dtype, np.floating):
            raise ValueError("cluster_rows: init must be %d row indices or a float [%d, %d] array of centroids, got shape %s"
                             % (k, k, dim, tuple(arr.shape)))
    What = _unit_rows(What_or_table, normalised, device)
    if init is None:
        usable = np.flatnonzero(usable_rows(What).cpu().numpy())
        if len(usable) < k:
            raise ValueError("cluster_rows: k = %d clusters but the table has only %d usable rows" % (k, len(usable)))
        init_rows = np.random.default_rng(seed).choice(usable, size=k, replace=False)
    C0 = What[torch.as_tensor(init_rows, device=What.device)] if init_rows is not None else \
        torch.as_tensor(np.ascontiguousarray(arr, np.float32), device=What.device)
    C, assign, sim, count, iters, converged = ops.kmeans_fit(What, C0, max_iter)
    return dict(C=C, assign=assign, sim=sim, count=count, iters=iters, converged=converged, init_rows=init_rows)


def assign_clusters(C, rows, normalised=None, device="cuda:0"):
    """The cluster of rows outside the fitted table — folded-in users, new anime — by an existing clustering, no refit:
    ``ops.kmeans_assign`` on ``rows`` (a device tensor: unit rows as they are; a host array: raw rows, normalised here;
    ``normalised`` says which instead) against the centroids ``C``.  Returns (assign int32, sim fp32) on the device."""
    from . import ops
    What = _unit_rows(rows, normalised, device)
    return ops.kmeans_assign(What, torch.as_tensor(C, device=What.device))


MAP_BISECT_STEPS = 64   # bisection steps of a row's bandwidth
MAP_QUERY_BATCH = 4096  # query rows of one cosine_topk call of the neighbour lists


def _map_bandwidths(d2, perplexity, steps=MAP_BISECT_STEPS):
    """p(j|i) over each row's neighbour distances ``d2`` fp64 [n, k] (any device): the precision beta of every row by
    ``steps`` bisection steps on the entropy of exp(-beta (d2 - min d2)) towards log(perplexity), the bracket [0, inf)
    doubled while it is open.  Plumbing in torch fp64 (it contains ``exp``: held to NumPy by tolerance, not by bits).
    Returns (p fp64 [n, k], rows summing to 1; beta fp64 [n])."""
    d2 = d2.to(torch.float64)
    n = d2.shape[0]
    target = float(np.log(np.float64(perplexity)))
    d0 = d2 - d2.min(dim=1, keepdim=True).values
    beta = torch.ones(n, dtype=torch.float64, device=d2.device)
    lo = torch.zeros_like(beta)
    hi = torch.full_like(beta, float("inf"))
    for _ in range(int(steps)):
        p = torch.exp(-d0 * beta[:, None])
        s = p.sum(dim=1)
        h = torch.log(s) + beta * (d0 * p).sum(dim=1) / s
        high = h > target                       # too flat: beta must grow
        lo = torch.where(high, beta, lo)
        hi = torch.where(high, hi, beta)
        beta = torch.where(torch.isinf(hi), beta * 2.0, (lo + hi) / 2.0)
    p = torch.exp(-d0 * beta[:, None])
    return p / p.sum(dim=1, keepdim=True), beta


def _map_symmetrise(nbr, p, n):
    """P' = p(j|i) + p(i|j) as a CSR over ``n`` rows (offsets int64 [n + 1], idx int32 ascending in a row, val fp32) from
    the neighbour lists ``nbr`` int [n, k] (-1 = none) and ``p`` fp64 [n, k], on their device.  Each value is the sum of
    at most two terms, so the order the adds land in cannot change it."""
    dev = nbr.device
    rows = torch.arange(n, device=dev).repeat_interleave(nbr.shape[1])
    cols = nbr.reshape(-1).long()
    vals = p.reshape(-1).to(torch.float64)
    keep = cols >= 0
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    key = torch.cat([rows * n + cols, cols * n + rows])
    uniq, inv = torch.unique(key, return_inverse=True)
    summed = torch.zeros(uniq.numel(), dtype=torch.float64, device=dev).index_add_(0, inv, torch.cat([vals, vals]))
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(torch.bincount(uniq // n, minlength=n), 0)
    return offsets, (uniq % n).to(torch.int32), summed.to(torch.float32)


def _map_neighbours(What, queries, k, keep=None):
    """(idx int32 [nq, k], cos fp32 [nq, k]) of the query rows' nearest rows by ``ops.cosine_topk`` (exclude_self set),
    a batch of query rows at a time"""
    from . import ops
    out = [ops.cosine_topk(What, queries[b:b + MAP_QUERY_BATCH], k, exclude_self=True, keep=keep)
           for b in range(0, int(queries.numel()), MAP_QUERY_BATCH)]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


def check_map(n_rows, perplexity, neighbours=None):
    """The argument checks of ``map_affinities`` on a table of ``n_rows`` usable rows (no device needed): (perplexity
    float, neighbours int), ``neighbours`` = None being min(n_rows - 1, 3 * perplexity).  ValueError for fewer than 2
    rows or more than TSNE_MAX_ROWS, ``neighbours`` outside 1 .. n_rows - 1, a perplexity outside [1, neighbours]."""
    n_rows, perplexity = int(n_rows), float(perplexity)
    if not 2 <= n_rows <= _lib.TSNE_MAX_ROWS:
        raise ValueError("map: a table of %d usable rows; a map takes 2 .. %d (TSNE_MAX_ROWS)"
                         % (n_rows, _lib.TSNE_MAX_ROWS))
    if not perplexity >= 1.0:
        raise ValueError("map: perplexity = %r must be at least 1" % perplexity)
    k = min(n_rows - 1, int(3 * perplexity)) if neighbours is None else int(neighbours)
    if not 1 <= k <= n_rows - 1:
        raise ValueError("map: neighbours = %d must be in 1 .. %d (the other usable rows)" % (k, n_rows - 1))
    if perplexity > k:
        raise ValueError("map: perplexity = %r cannot exceed the %d neighbours of a row" % (perplexity, k))
    return perplexity, k


def map_affinities(What_or_table, perplexity=30.0, neighbours=None, normalised=None, device="cuda:0"):
    """The t-SNE affinities of an embedding table: for every usable row (``usable_rows``) its
    ``neighbours`` nearest usable rows by the exact ``ops.cosine_topk`` (default min(n - 1, 3 * perplexity)), d^2 = 2 -
    2 cos on the unit rows, the row's bandwidth by 64 bisection steps towards ``perplexity``, symmetrised to P'_ij =
    p(j|i) + p(i|j).  ``What_or_table`` as ``cluster_rows`` takes it.
    Returns a dict: rows int64 [m] (the usable rows of the table, ascending: the CSR's row r is table row rows[r]),
    offsets int64 [m + 1], idx int32, val fp32 (device tensors), beta fp64 [m], n_rows, perplexity, neighbours, What (the
    unit rows).  Raises ValueError as ``check_map`` does."""
    if len(tuple(What_or_table.shape)) != 2:
        raise ValueError("map_affinities: a table must be [n_rows, width]")
    _lib.check_width(What_or_table.shape[1])
    check_map(What_or_table.shape[0], perplexity, neighbours)      # the refusals that need no device come first
    What = _unit_rows(What_or_table, normalised, device)
    rows = torch.nonzero(usable_rows(What)).reshape(-1)
    m = int(rows.numel())
    perplexity, k = check_map(m, perplexity, neighbours)
    Wu = What if m == What.shape[0] else What[rows].contiguous()
    nbr, cos = _map_neighbours(Wu, torch.arange(m, device=What.device, dtype=torch.int32), k)
    p, beta = _map_bandwidths(2.0 - 2.0 * cos.to(torch.float64), perplexity)
    offsets, idx, val = _map_symmetrise(nbr, p, m)
    return dict(rows=rows, offsets=offsets, idx=idx, val=val, beta=beta, n_rows=int(What.shape[0]),
                perplexity=perplexity, neighbours=k, What=What)


def map_lr(n_rows, exaggeration=12.0):
    """scikit-learn's automatic learning rate: max(n / exaggeration / 4, 50)"""
    return max(float(n_rows) / float(exaggeration) / 4.0, 50.0)


def map_kl(Y, offsets, idx, val):
    """KL(P || Q) of the map ``Y`` [m, 2] under the CSR affinities (P = P' / (2 m)), torch fp64 in row chunks; for
    reporting only."""
    Y = Y.to(torch.float64)
    m = int(Y.shape[0])
    Z = torch.zeros((), dtype=torch.float64, device=Y.device)
    chunk = max(1, (1 << 24) // m)
    for b in range(0, m, chunk):
        d2 = (Y[b:b + chunk, None, :] - Y[None, :, :]).square().sum(dim=2)
        Z += (1.0 / (1.0 + d2)).sum() - min(chunk, m - b)     # the self pairs: q = 1 each
    r = torch.arange(m, device=Y.device).repeat_interleave(offsets[1:] - offsets[:-1])
    q = 1.0 / (1.0 + (Y[r] - Y[idx.long()]).square().sum(dim=1))
    P = val.to(torch.float64) / (2.0 * m)
    ok = P > 0
    return float((P[ok] * torch.log(P[ok] * Z / q[ok])).sum())


def map_rows(What_or_table, perplexity=30.0, iters=1000, exag_iters=250, exaggeration=12.0, lr=None, seed=0, init=None,
             affinities=None, normalised=None, device="cuda:0"):
    """A two-dimensional map of an embedding table by exact t-SNE (``ops.tsne_fit``): the same seed
    gives the same bits.  ``affinities``: a ``map_affinities`` result (None computes it with ``perplexity``).
    Y0 = 1e-4 * ``np.random.default_rng(seed).standard_normal((n_rows, 2))`` as fp32 unless ``init`` [n_rows, 2] is
    given; ``lr`` = None is scikit-learn's rule max(m / exaggeration / 4, 50) over the m usable rows.
    Returns a dict: Y fp32 [n_rows, 2] on the device, centred over the usable rows, NaN for a row that is not usable;
    kl (the final KL divergence, float); info (``ops.tsne_fit``'s bits); lr, iters, seed, affinities."""
    from . import ops
    shape = tuple(What_or_table.shape)
    ops.check_tsne(max(1, min(shape[0], _lib.TSNE_MAX_ROWS)), iters, exag_iters, exaggeration, 1.0 if lr is None else lr)
    if init is not None and tuple(np.shape(init)) != (shape[0], 2):
        raise ValueError("map_rows: init must be [%d, 2], got %s" % (shape[0], tuple(np.shape(init))))
    aff = affinities if affinities is not None else map_affinities(What_or_table, perplexity, None, normalised, device)
    if aff["n_rows"] != shape[0]:
        raise ValueError("map_rows: affinities of a table of %d rows, not %d" % (aff["n_rows"], shape[0]))
    rows, dev = aff["rows"], aff["offsets"].device
    m = int(rows.numel())
    lr = map_lr(m, exaggeration) if lr is None else float(lr)
    if init is None:
        Y0 = (1e-4 * np.random.default_rng(seed).standard_normal((shape[0], 2))).astype(np.float32)
    else:
        Y0 = np.ascontiguousarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init, np.float32)
    Y0 = torch.as_tensor(Y0, device=dev)[rows].contiguous()
    Ym, _, _, info = ops.tsne_fit(Y0, aff["offsets"], aff["idx"], aff["val"], iters, exag_iters, exaggeration, lr)
    kl = map_kl(Ym, aff["offsets"], aff["idx"], aff["val"])
    Ym = (Ym.to(torch.float64) - Ym.to(torch.float64).mean(dim=0, keepdim=True)).to(torch.float32)
    Y = torch.full((shape[0], 2), float("nan"), dtype=torch.float32, device=dev)
    Y[rows] = Ym
    return dict(Y=Y, kl=kl, info=info, lr=lr, iters=int(iters), seed=seed, affinities=aff)


def _map_place_positions(Y, nbr, cos, perplexity):
    """The positions of placed rows: the p(j|row)-weighted mean (fp64) of the map positions ``Y`` [m, 2] of each row's
    neighbours ``nbr`` int [r, k] with the cosines ``cos`` [r, k]; the bandwidth code of the fit.  fp32 [r, 2]."""
    p, _ = _map_bandwidths(2.0 - 2.0 * cos.to(torch.float64), perplexity)
    return (p[:, :, None] * Y.to(torch.float64)[nbr.long()]).sum(dim=1).to(torch.float32)


def map_place(fit, rows, normalised=None, device="cuda:0"):
    """The map positions of rows outside the fitted table — folded-in users, new anime — by a ``map_rows`` result, no
    refit: a placed row sits at the affinity-weighted mean of the map positions of its nearest fitted rows (the
    neighbour count, perplexity and bandwidth code of the fit).  ``rows`` as ``assign_clusters`` takes them.  Returns
    fp32 [n, 2] on the device, NaN for a row that is not usable."""
    aff = fit["affinities"]
    What, used = aff["What"], aff["rows"]
    R = _unit_rows(rows, normalised, device)
    if R.shape[1] != What.shape[1]:
        raise ValueError("map_place: rows of width %d on a map of width %d" % (R.shape[1], What.shape[1]))
    ok = torch.nonzero(usable_rows(R)).reshape(-1)
    out = torch.full((int(R.shape[0]), 2), float("nan"), dtype=torch.float32, device=What.device)
    if ok.numel() == 0:
        return out
    m = int(used.numel())
    stacked = torch.cat([What[used], R[ok]]).contiguous()
    keep = torch.zeros(stacked.shape[0], dtype=torch.uint8, device=What.device)
    keep[:m] = 1                                                  # neighbours among the fitted rows only
    q = torch.arange(m, m + int(ok.numel()), device=What.device, dtype=torch.int32)
    nbr, cos = _map_neighbours(stacked, q, aff["neighbours"], keep)
    out[ok] = _map_place_positions(fit["Y"][used], nbr, cos, aff["perplexity"])
    return out


FOLD_STEPS = 100        # Adam iterations of a fold-in
FOLD_LR = 0.01          # and their learning rate


def _fold_csr(fn, new, other, rat, held_ids, table_ids, known_msg):
    """The CSR of rating triples grouped by ``new`` (ids in order of first appearance, each list in input order,
    repeats kept), the ``other`` ids encoded as rows of ``table_ids`` and dropped (and counted) where it has none.
    ValueError (prefixed ``fn``) for a rating that is NaN or outside [0, 1] and, with ``known_msg``, for ``new`` ids
    that ``held_ids`` already holds."""
    from .data import encode_ids
    new = np.asarray(new).astype(np.int64)
    other = np.asarray(other).astype(np.int64)
    rat = np.asarray(rat, np.float32)
    if len(rat) and not bool(np.all((rat >= 0) & (rat <= 1))):      # (a NaN fails both comparisons)
        raise ValueError("%s: ratings must be numbers in [0, 1] (the preprocess step's scaled ratings); "
                         "%d of %d are not" % (fn, int((~((rat >= 0) & (rat <= 1))).sum()), len(rat)))
    row, new_ids = encode_ids(new)
    new_ids = np.asarray(new_ids, np.int64)
    known = new_ids[np.isin(new_ids, np.asarray(held_ids, np.int64))]
    if len(known):
        raise ValueError(fn + ": " + known_msg % ", ".join(str(int(x)) for x in known[:20]))
    table_ids = np.asarray(table_ids, np.int64)
    order = np.argsort(table_ids, kind="stable")
    pos = np.searchsorted(table_ids[order], other)
    pos[pos == len(table_ids)] = 0
    has = (table_ids[order][pos] == other) if len(table_ids) else np.zeros(len(other), bool)
    n_dropped = int((~has).sum())
    row, t_idx, rat = np.asarray(row, np.int64)[has], order[pos][has].astype(np.int32), rat[has]
    by_row = np.argsort(row, kind="stable")
    offsets = np.zeros(len(new_ids) + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=len(new_ids)), out=offsets[1:])
    return new_ids, offsets, np.ascontiguousarray(t_idx[by_row]), np.ascontiguousarray(rat[by_row]), n_dropped


def fold_in_csr(frame, user_ids, anime_ids):
    """Host half of ``fold_in_users``: the CSR of a rating frame (``user_id, anime_id, rating``: the preprocess output
    schema, rating in [0, 1]).  Users come in the order of their first appearance, each user's ratings in frame order
    (repeats stay); ratings of anime outside ``anime_ids`` (the model has no row for them) are dropped and counted.
    Returns (new_ids int64 [n_new], offsets int64 [n_new + 1], anime_idx int32 [nnz], rating fp32 [nnz], n_dropped).
    ValueError, naming them, for user ids ``user_ids`` (the model's) already holds, and for a rating that is NaN or
    outside [0, 1]."""
    return _fold_csr("fold_in_users", frame["user_id"], frame["anime_id"], frame["rating"], user_ids, anime_ids,
                     "user id(s) %s already have an embedding row in the model (use model_recs for them)")


def fold_in_anime_csr(frame, user_ids, anime_ids):
    """Host half of ``fold_in_anime``, ``fold_in_csr`` with the roles swapped: the CSR by ``anime_id`` of the frame, the
    anime in the order of their first appearance, each list in frame order; ratings by users outside ``user_ids`` are
    dropped and counted.  Returns (new_ids int64 [n_new], offsets int64 [n_new + 1], user_idx int32 [nnz], rating fp32
    [nnz], n_dropped).  ValueError, naming them, for anime ids ``anime_ids`` (the model's) already holds, and for a
    rating that is NaN or outside [0, 1]."""
    return _fold_csr("fold_in_anime", frame["anime_id"], frame["user_id"], frame["rating"], anime_ids, user_ids,
                     "anime id(s) %s already have an embedding row in the model (similar_anime and model_recs serve them)")


def fold_in_users(model, frame, steps=FOLD_STEPS, lr=FOLD_LR, l2=1e-4, init=None, device="cuda:0"):
    """Embedding rows for the users of ``frame`` (``user_id, anime_id, rating`` in [0, 1]), none of whom the model
    (``weights_io.load_model``'s dict) was trained on: ``ops.fold_in`` on their ratings, with the model's own head,
    activation and loss (binary_crossentropy when the file records none).  ``init``: the start row(s); by default the
    fp32 mean row of ``model["U"]``.  Returns dict(ids int64 [n_new], rows fp32 [n_new, width] and loss fp32 [n_new]
    on the device, watched int32 [n_new, ceil(n_anime/32)]: the bits ``ops.seen_bits`` sets for the ratings kept,
    n_dropped: ratings of anime the model has no row for, offsets / anime_idx / rating: the CSR that was fitted)."""
    from . import ops, weights_io
    if model.get("user_ids") is None or model.get("anime_ids") is None:
        raise ValueError("fold_in_users: the model file has no id tables")
    ids, offsets, a_idx, rat, n_dropped = fold_in_csr(frame, model["user_ids"], model["anime_ids"])
    A = torch.as_tensor(np.ascontiguousarray(model["A"], np.float32), device=device)
    if init is None:
        init = np.asarray(model["U"], np.float32).mean(axis=0, dtype=np.float32)
    rows, loss = ops.fold_in(A, weights_io.model_head(model), offsets, a_idx, rat, init, lr=lr, steps=steps, l2=l2,
                             loss=model.get("loss") or "binary_crossentropy")
    u_idx = np.repeat(np.arange(len(ids), dtype=np.int32), np.diff(offsets))
    watched = ops.seen_bits(u_idx, a_idx, len(ids), A.shape[0], device=device)
    return {"ids": ids, "rows": rows, "loss": loss, "watched": watched, "n_dropped": n_dropped, "offsets": offsets,
            "anime_idx": a_idx, "rating": rat}


def fold_in_anime(model, frame, steps=FOLD_STEPS, lr=FOLD_LR, l2=1e-4, init=None, device="cuda:0"):
    """Embedding rows for the anime of ``frame`` (``user_id, anime_id, rating`` in [0, 1]) that the model holds no row
    for, from the ratings users it does hold gave them: ``ops.fold_in_split`` against the frozen ``model["U"]`` with the
    model's own head, activation and loss.  ``init``: the start row(s); by default the fp32 mean row of ``model["A"]``.
    Returns dict(ids int64 [n_new], rows fp32 [n_new, width] and loss fp32 [n_new] on the device, rated int32
    [n_new, ceil(n_users/32)]: the bits ``ops.seen_bits`` sets for the users whose ratings were kept, n_dropped:
    ratings by users the model has no row for, offsets / user_idx / rating: the CSR that was fitted)."""
    from . import ops, weights_io
    if model.get("user_ids") is None or model.get("anime_ids") is None:
        raise ValueError("fold_in_anime: the model file has no id tables")
    ids, offsets, u_idx, rat, n_dropped = fold_in_anime_csr(frame, model["user_ids"], model["anime_ids"])
    U = torch.as_tensor(np.ascontiguousarray(model["U"], np.float32), device=device)
    if init is None:
        init = np.asarray(model["A"], np.float32).mean(axis=0, dtype=np.float32)
    rows, loss = ops.fold_in_split(U, weights_io.model_head(model), offsets, u_idx, rat, init, lr=lr, steps=steps, l2=l2,
                                   loss=model.get("loss") or "binary_crossentropy")
    a_row = np.repeat(np.arange(len(ids), dtype=np.int32), np.diff(offsets))
    rated = ops.seen_bits(a_row, u_idx, len(ids), U.shape[0], device=device)
    return {"ids": ids, "rows": rows, "loss": loss, "rated": rated, "n_dropped": n_dropped, "offsets": offsets,
            "user_idx": u_idx, "rating": rat}


def append_anime(model, folded):
    """The model dict with the folded anime (``fold_in_anime``'s result) at the end of ``A`` and ``anime_ids``; every
    other entry is the model's own object.  Written with ``weights_io.save_model`` it is a model file that
    similar_anime and model_recs serve the new anime from as they are."""
    rows = folded["rows"]
    rows = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    out = dict(model)
    out["A"] = np.concatenate([np.asarray(model["A"], np.float32), rows.astype(np.float32)])
    ids = np.asarray(model["anime_ids"])
    out["anime_ids"] = np.concatenate([ids, np.asarray(folded["ids"]).astype(ids.dtype)])
    return out


# ----------------------------------------------------------------------------------------
# the score-row driver: any system's lists and ranks, a span of lists at a time
# ----------------------------------------------------------------------------------------
def _spans(n_lists, batch, what):
    n_lists, batch = int(n_lists), int(batch)
    if batch < 1:
        raise ValueError("%s: batch must be >= 1" % what)
    return [(l0, min(n_lists, l0 + batch)) for l0 in range(0, n_lists, batch)]


def _span_rows(source, l0, l1):
    """the score rows fp32 [l1 - l0, n_anime] of a span: a callable source is asked for them, a 1-D vector is every
    list's row"""
    return source(l0, l1) if callable(source) else source.reshape(1, -1).expand(l1 - l0, -1)


def _span_bits(watched_bits, l0, l1):
    return None if watched_bits is None else watched_bits[l0:l1]


def _targets(what, target_row, target_anime, n_lists, unwatched=None):
    """(target_row, target_anime) as int64 host arrays, or a ValueError that starts with ``what``: another length, a
    target_row outside 0 .. n_lists - 1 and, with ``unwatched`` (watched bits [n_lists, words] on any device), a
    target_anime past its words or a target whose own bit is set there."""
    tr = np.asarray(_host(target_row), np.int64).reshape(-1)
    ta = np.asarray(_host(target_anime), np.int64).reshape(-1)
    if tr.shape != ta.shape:
        raise ValueError("%s: target_row and target_anime must have one entry per target" % what)
    if tr.size and (tr.min() < 0 or tr.max() >= int(n_lists)):
        raise ValueError("%s: target_row out of range" % what)
    if unwatched is not None and tr.size:
        if ta.min() < 0 or ta.max() >= 32 * int(unwatched.shape[1]):
            raise ValueError("%s: target_anime out of range" % what)
        words = _host(unwatched[torch.as_tensor(tr, device=unwatched.device),
                                torch.as_tensor(ta >> 5, device=unwatched.device)]).astype(np.int64)
        if ((words >> (ta & 31)) & 1).any():
            raise ValueError("%s: a target has its own watched bit set (a fused row holds no value there)" % what)
    return tr, ta


def rows_topk_batched(source, n_lists, k, watched_bits=None, keep=None, batch=4096, what="rows_topk_batched",
                      device=None):
    """The ``k`` best anime of each of ``n_lists`` lists by the score rows of ``source`` — a callable ``(l0, l1) -> fp32
    [l1 - l0, n_anime]`` on the device, or a 1-D vector shared by every list — without a bit in ``watched_bits``
    [n_lists, ceil(n_anime/32)] and with ``keep`` [n_anime] set, by the exact select (``ops.rows_topk``), ``batch`` lists
    at a time.  Returns (idx int32 [n_lists, k], score fp32 [n_lists, k]) on ``device`` (None: where the select leaves
    them; the host when there is no list).  ValueError, starting with ``what``, for ``batch`` < 1."""
    from . import ops
    n_lists, k = int(n_lists), int(k)
    out = None if device is None else (torch.empty(n_lists, k, dtype=torch.int32, device=device),
                                       torch.empty(n_lists, k, dtype=torch.float32, device=device))
    for l0, l1 in _spans(n_lists, batch, what):
        i, s = ops.rows_topk(_span_rows(source, l0, l1), k, keep=keep, wbits=_span_bits(watched_bits, l0, l1))
        if out is None:
            out = (torch.empty(n_lists, k, dtype=torch.int32, device=i.device),
                   torch.empty(n_lists, k, dtype=torch.float32, device=i.device))
        out[0][l0:l1], out[1][l0:l1] = i, s
    return out if out is not None else (torch.empty(0, k, dtype=torch.int32), torch.empty(0, k, dtype=torch.float32))


def rows_rank_batched(source, n_lists, watched_bits, target_row, target_anime, batch=4096, what="rows_rank_batched",
                      device=None, own_bit_clear=False):
    """The ranks ``ops.predict_rank`` gives a model, for the score rows of ``source`` (as ``rows_topk_batched`` takes
    it): target t is (``target_row[t]``: a list, ``target_anime[t]``); returns rank int32 [n_t] on ``device`` (None:
    where ``ops.rows_rank`` leaves them; the host without targets): 0 = first among the anime the list has no watched bit
    for, the target's own bit ignored.  ``batch`` lists at a time; a span that holds no target is not scored.
    ValueError, starting with ``what``, for ``batch`` < 1, targets of two lengths, a target_row out of range and, with
    ``own_bit_clear``, a target whose own watched bit is set."""
    from . import ops
    spans = _spans(n_lists, batch, what)
    tr, ta = _targets(what, target_row, target_anime, n_lists, watched_bits if own_bit_clear else None)
    rank = None if device is None else torch.empty(int(tr.size), dtype=torch.int32, device=device)
    for l0, l1 in spans:
        sel = np.flatnonzero((tr >= l0) & (tr < l1))
        if not sel.size:
            continue
        r = ops.rows_rank(_span_rows(source, l0, l1), tr[sel] - l0, ta[sel], _span_bits(watched_bits, l0, l1))
        if rank is None:
            rank = torch.empty(int(tr.size), dtype=torch.int32, device=r.device)
        rank[torch.as_tensor(sel, device=rank.device)] = r
    return torch.empty(0, dtype=torch.int32) if rank is None else rank


# ----------------------------------------------------------------------------------------
# item-kNN from co-occurrence: no model takes part
# ----------------------------------------------------------------------------------------
COOC_BATCH = 1024       # query items per anirec_cooc_scores call: a sim row and a count row each
ITEMKNN_BATCH = 4096    # users per anirec_itemknn_scores call: a score row each


def item_bits(user_idx, anime_idx, n_users, n_anime, device="cuda:0"):
    """The liked-by bits of a rating list: int32 [n_anime, ceil(n_users/32)], bit ``u & 31`` of word ``u >> 5`` of row a
    set for every rating (u, a) — ``ops.seen_bits`` with the two columns swapped, the ``bits`` of ``ops.cooc_scores``.
    Raises ValueError on an index out of range."""
    from . import ops
    return ops.seen_bits(anime_idx, user_idx, n_anime, n_users, device=device)


def cooc_neighbours(bits, n_users, k, queries=None, measure="cosine", shrink=0.0, min_support=1, batch=COOC_BATCH):
    """The ``k`` nearest items of each query item by co-occurrence (``ops.cooc_scores`` then ``ops.rows_topk`` with the
    scores' own ``excl`` rows as the mask, ``batch`` queries at a time): ``bits`` as ``item_bits`` gives them,
    ``queries`` item indices (None: every item).  Returns (idx int32 [nq, k], sim fp32 [nq, k], count int32 [nq, k]) on
    the device: larger similarity first, ties by index, never the query itself nor an item below the support; padded
    with -1 / NaN / -1.  ``count`` is the number of users who liked both."""
    from . import ops
    k, batch = int(k), int(batch)
    if k < 1 or batch < 1:
        raise ValueError("cooc_neighbours: k and batch must be >= 1")
    ops.check_cooc(measure, shrink, min_support)
    dev = bits.device
    n = int(bits.shape[0])
    q = torch.arange(n, dtype=torch.int32, device=dev) if queries is None else \
        torch.as_tensor(_host(queries) if not isinstance(queries, torch.Tensor) else queries, device=dev) \
        .to(torch.int32).reshape(-1)
    nq = int(q.numel())
    idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
    sim = torch.empty(nq, k, dtype=torch.float32, device=dev)
    cnt = torch.empty(nq, k, dtype=torch.int32, device=dev)
    for q0 in range(0, nq, batch):
        s, c, ex, _ = ops.cooc_scores(bits, n_users, q[q0:q0 + batch], measure, shrink, min_support, count=True, excl=True)
        i, v = ops.rows_topk(s, k, wbits=ex)
        idx[q0:q0 + batch], sim[q0:q0 + batch] = i, v
        cnt[q0:q0 + batch] = torch.where(i >= 0, torch.gather(c, 1, i.clamp(min=0).long()), torch.full_like(i, -1))
    return idx, sim, cnt


def itemknn_fit(user_idx, anime_idx, rating, n_users, n_anime, liked_min_rating=0.0, K=50, measure="cosine", shrink=0.0,
                min_support=1, device="cuda:0"):
    """An item-kNN model from a rating list: a user LIKED an anime when the (scaled) rating is at or above
    ``liked_min_rating`` (compared in fp32; 0.0 = every rating); every anime keeps its ``K`` nearest by co-occurrence of
    the liked-by sets (``cooc_neighbours``).  Returns {"nbr_idx" int32 [n_anime, K], "nbr_sim" fp32, "nbr_count" int32,
    "pop" int32 [n_anime] (how many users liked each anime)} on the device and the parameters ("n_users", "n_anime",
    "K", "measure", "shrink", "min_support", "liked_min_rating")."""
    from . import ops
    u, a = _host(user_idx).reshape(-1), _host(anime_idx).reshape(-1)
    r = _host(rating).reshape(-1).astype(np.float32)
    if not len(u) == len(a) == len(r):
        raise ValueError("itemknn_fit: user_idx, anime_idx and rating must have one entry per rating")
    liked = r >= np.float32(liked_min_rating)
    dev = torch.device(device)
    bits = item_bits(torch.as_tensor(u[liked].astype(np.int32), device=dev),
                     torch.as_tensor(a[liked].astype(np.int32), device=dev), n_users, n_anime, device=dev)
    idx, sim, cnt = cooc_neighbours(bits, n_users, K, None, measure, shrink, min_support)
    pop = ops.cooc_scores(bits, n_users, [0], measure, shrink, min_support, pop=True)[3]
    return {"nbr_idx": idx, "nbr_sim": sim, "nbr_count": cnt, "pop": pop, "n_users": int(n_users),
            "n_anime": int(n_anime), "K": int(K), "measure": str(measure).strip().lower(), "shrink": float(shrink),
            "min_support": int(min_support), "liked_min_rating": float(liked_min_rating)}


def _on(x, dev, dtype):
    """``x`` (NumPy or torch, wherever it lives) as a tensor of ``dtype`` on ``dev``"""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=dev, dtype=dtype)


def _knn_source(knn, offsets, hist_idx, hist_w):
    """(the row source of ``itemknn_rows_source``, n_lists)"""
    from . import ops
    off = np.asarray(_host(offsets), np.int64).reshape(-1)
    if off.size < 1:
        raise ValueError("itemknn: offsets holds n_lists + 1 entries")
    dev = knn["nbr_idx"].device
    hi = _on(hist_idx, dev, torch.int32)
    hw = None if hist_w is None else _on(hist_w, dev, torch.float32)
    return lambda l0, l1: ops.itemknn_scores(knn["nbr_idx"], knn["nbr_sim"], off[l0:l1 + 1], hi, hw), int(off.size) - 1


def itemknn_topk(knn, offsets, hist_idx, hist_w=None, k=10, watched_bits=None, batch=ITEMKNN_BATCH):
    """Item-kNN recommendation lists: list l's history ``hist_idx[offsets[l]:offsets[l + 1]]`` (``history_csr`` builds
    it; ``hist_w`` None = weight 1) scored through the neighbour tables of ``knn`` (``ops.itemknn_scores``) and the
    ``k`` best anime without a bit in ``watched_bits`` [n_lists, ceil(n_anime/32)] taken by the exact select
    (``ops.rows_topk``), ``batch`` lists at a time.  Returns (idx int32 [n_lists, k], score fp32 [n_lists, k])."""
    source, n_l = _knn_source(knn, offsets, hist_idx, hist_w)
    return rows_topk_batched(source, n_l, k, watched_bits, None, batch, "itemknn_topk", knn["nbr_idx"].device)


def itemknn_rank(knn, offsets, hist_idx, hist_w, watched_bits, target_row, target_anime, batch=ITEMKNN_BATCH):
    """The ranks ``ops.predict_rank`` gives a model, for the item-kNN scores of ``itemknn_topk``: target t is
    (``target_row[t]``: a list, ``target_anime[t]``); returns rank int32 [n_t] on the device (0 = first among the anime
    the list has no watched bit for, the target's own bit ignored).  ``batch`` lists at a time."""
    source, n_l = _knn_source(knn, offsets, hist_idx, hist_w)
    return rows_rank_batched(source, n_l, watched_bits, target_row, target_anime, batch, "itemknn_rank",
                             knn["nbr_idx"].device)


# ----------------------------------------------------------------------------------------
# content-based lists from the metadata: no model and no rating of the listed anime takes part
# ----------------------------------------------------------------------------------------
CONTENT_SYSTEMS = ("content",)  # row-score systems beside HYBRID_SYSTEMS (which stays as it is): hybrid members too
CONTENT_COLUMNS = ("Genres", "Type", "Source", "Studios", "Rating")
CONTENT_SYNOPSIS = "Sypnopsis"  # the opt-in text column (metadata_by_index's spelling)
CONTENT_WEIGHTS = ("rating", "centered", "one")
CONTENT_BATCH = 4096            # users per anirec_content_scores call: a score row each
CONTENT_WS_BYTES = 1 << 30      # the batch shrinks until the call's workspace (its global form) fits in this


def check_content_fit(columns=CONTENT_COLUMNS, min_df=1, max_df=1.0):
    """(columns as a tuple, min_df, max_df), or a ValueError before any GPU use: no column, a column twice, a column
    that is neither one of CONTENT_COLUMNS nor the synopsis, ``min_df`` < 1 or ``max_df`` outside (0, 1]."""
    cols = [columns] if isinstance(columns, str) else list(columns)
    cols = [str(c).strip() for c in cols]
    known = CONTENT_COLUMNS + (CONTENT_SYNOPSIS,)
    for c in cols:
        if c not in known:
            raise ValueError("content column %r is not one of %s" % (c, ", ".join(known)))
    if not cols or len(set(cols)) != len(cols):
        raise ValueError("content columns %r must be one or more distinct names of %s" % (cols, ", ".join(known)))
    min_df, max_df = int(min_df), float(max_df)
    if min_df < 1 or not 0.0 < max_df <= 1.0:
        raise ValueError("content_fit: min_df = %r must be >= 1 and max_df = %r in (0, 1]" % (min_df, max_df))
    return tuple(cols), min_df, max_df


def content_rows(meta, columns=CONTENT_COLUMNS, min_df=1, max_df=1.0):
    """The TF-IDF rows of ``content_fit`` on the host: (vocab, rows) — the sorted token strings and, per row of ``meta``,
    (token ids ascending int32, weights fp32)."""
    import math
    import re
    from collections import Counter
    from .components import category_tokens
    cols, min_df, max_df = check_content_fit(columns, min_df, max_df)
    for c in cols:
        if c not in meta.columns:
            raise ValueError("content_fit: the metadata frame has no column %r" % c)
    n = len(meta)
    tf = [{} for _ in range(n)]
    for c in cols:
        cells = meta[c].tolist()
        if c == CONTENT_SYNOPSIS:
            counts = [Counter(re.findall(r"[a-z]{3,}", cell.lower())) if isinstance(cell, str) and cell != "None"
                      else Counter() for cell in cells]
            df = Counter(t for cnt in counts for t in cnt)
            kept = {t for t, d in df.items() if min_df <= d <= max_df * n}
            for row, cnt in zip(tf, counts):
                for t, k in cnt.items():
                    if t in kept:
                        row[c + "=" + t] = 1.0 + math.log(k)
        else:
            for row, cell in zip(tf, cells):
                for t in category_tokens(cell):
                    if t:
                        row[c + "=" + t] = 1.0
    vocab = sorted({t for row in tf for t in row})
    index = {t: i for i, t in enumerate(vocab)}
    df = Counter(t for row in tf for t in row)
    idf = {t: math.log((1.0 + n) / (1.0 + df[t])) + 1.0 for t in vocab}
    rows = []
    for row in tf:
        toks = sorted(row, key=index.__getitem__)
        w = [row[t] * idf[t] for t in toks]
        norm = math.sqrt(math.fsum(x * x for x in w))        # the correctly rounded sum: no order to restate
        rows.append((np.asarray([index[t] for t in toks], np.int32), np.asarray([x / norm for x in w], np.float32)))
    return vocab, rows


def content_fit(meta, columns=CONTENT_COLUMNS, min_df=1, max_df=1.0, device="cuda:0"):
    """TF-IDF item vectors from the metadata, on the host (NumPy and pandas alone): ``meta`` a frame aligned with the
    caller's item index (``components.metadata_by_index``), ``columns`` of CONTENT_COLUMNS and, opt-in, "Sypnopsis".
    A categorical cell is split by ``components.category_tokens``, each token prefixed with its column
    ("Genres=Action"; the same word in two columns is two tokens), tf 1.  A synopsis cell is lower-cased and tokenised
    by ``re.findall(r"[a-z]{3,}")``, tf = 1 + ln(count); only these tokens pass the document-frequency filter ``min_df``
    <= df <= ``max_df`` * n.  idf = ln((1 + n) / (1 + df)) + 1; a row is tf * idf, L2-normalised in fp64 and rounded to
    fp32; token ids ascend within a row, the vocabulary is sorted, a row without metadata (NaN cells) is empty.
    Returns {"tok_offsets" int64 [n_items + 1], "tok_idx" int32, "tok_w" fp32} on ``device``, "vocab" (the token
    strings), "n_items", "n_tokens" (at least 1) and the parameters ("columns", "min_df", "max_df").  ValueError, before
    any GPU use, as ``check_content_fit`` and for a column the frame lacks."""
    cols, min_df, max_df = check_content_fit(columns, min_df, max_df)
    vocab, rows = content_rows(meta, cols, min_df, max_df)
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(i) for i, _ in rows], out=off[1:])
    idx = np.concatenate([i for i, _ in rows]) if rows else np.zeros(0, np.int32)
    w = np.concatenate([x for _, x in rows]) if rows else np.zeros(0, np.float32)
    dev = torch.device(device)
    return {"tok_offsets": torch.as_tensor(off, device=dev), "tok_idx": torch.as_tensor(idx.astype(np.int32), device=dev),
            "tok_w": torch.as_tensor(w.astype(np.float32), device=dev), "vocab": vocab, "n_items": len(rows),
            "n_tokens": max(1, len(vocab)), "columns": cols, "min_df": min_df, "max_df": max_df}


def content_history_weights(rating, mode="rating", offsets=None):
    """The history weights of a content profile, fp32 on the host, one per rating: ``rating`` the rating itself,
    ``one`` 1, ``centered`` the rating minus the mean of its own list's ratings (``offsets``: the history CSR; None: one
    list), mean and difference in fp32 — a title rated below the user's mean pushes the profile away from its tokens.
    ValueError for a mode that is not one of CONTENT_WEIGHTS."""
    mode = str(mode).strip().lower()
    if mode not in CONTENT_WEIGHTS:
        raise ValueError("content_weight %r is not one of %s" % (mode, ", ".join(CONTENT_WEIGHTS)))
    r = _host(rating).reshape(-1).astype(np.float32)
    if mode == "one":
        return np.ones_like(r)
    if mode == "rating":
        return r
    off = np.asarray([0, len(r)] if offsets is None else _host(offsets), np.int64).reshape(-1)
    out = np.empty_like(r)
    for lo, hi in zip(off[:-1], off[1:]):
        if hi > lo:
            out[lo:hi] = r[lo:hi] - r[lo:hi].mean(dtype=np.float32)
    return out


def content_batch(fit, batch=CONTENT_BATCH):
    """The lists per ``ops.content_scores`` call: ``batch``, fewer where the call's workspace (n_tokens * 8 bytes a list
    above ``anirec_content_lds_tokens()``) would pass CONTENT_WS_BYTES."""
    return max(1, min(int(batch), CONTENT_WS_BYTES // (8 * int(fit["n_tokens"]))))


def _content_source(fit, offsets, hist_idx, hist_w):
    """(the row source of ``content_rows_source``, n_lists)"""
    from . import ops
    off = np.asarray(_host(offsets), np.int64).reshape(-1)
    if off.size < 1:
        raise ValueError("content: offsets holds n_lists + 1 entries")
    dev = fit["tok_offsets"].device
    hi = _on(hist_idx, dev, torch.int32)
    hw = None if hist_w is None else _on(hist_w, dev, torch.float32)
    step = content_batch(fit)

    def rows(l0, l1):       # a span of any driver, in calls whose workspace fits
        parts = [ops.content_scores(fit["tok_offsets"], fit["tok_idx"], fit["tok_w"], fit["n_tokens"],
                                    off[a:min(l1, a + step) + 1], hi, hw) for a in range(l0, max(l1, l0 + 1), step)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)
    return rows, int(off.size) - 1


def content_rows_source(fit, offsets, hist_idx, hist_w=None):
    """A row source of the content scores of the lists ``content_topk`` takes, through ``ops.content_scores``."""
    return _content_source(fit, offsets, hist_idx, hist_w)[0]


def content_topk(fit, offsets, hist_idx, hist_w=None, k=10, watched_bits=None, keep=None, batch=CONTENT_BATCH):
    """Content-based recommendation lists: list l's history ``hist_idx[offsets[l]:offsets[l + 1]]`` (``history_csr``
    builds it; ``hist_w`` None = weight 1, ``content_history_weights`` gives the others) scored against the item
    vectors of ``fit`` (``ops.content_scores``) and the ``k`` best items without a bit in ``watched_bits`` [n_lists,
    ceil(n_items/32)] and with ``keep`` [n_items] set taken by the exact select (``ops.rows_topk``), ``content_batch``
    lists at a time.  Returns (idx int32 [n_lists, k], score fp32 [n_lists, k])."""
    source, n_l = _content_source(fit, offsets, hist_idx, hist_w)
    return rows_topk_batched(source, n_l, k, watched_bits, keep, content_batch(fit, batch), "content_topk",
                             fit["tok_offsets"].device)


def content_rank(fit, offsets, hist_idx, hist_w, watched_bits, target_row, target_anime, batch=CONTENT_BATCH):
    """The ranks ``ops.predict_rank`` gives a model, for the content scores of ``content_topk``: target t is
    (``target_row[t]``: a list, ``target_anime[t]``); returns rank int32 [n_t] on the device (0 = first among the items
    the list has no watched bit for, the target's own bit ignored)."""
    source, n_l = _content_source(fit, offsets, hist_idx, hist_w)
    return rows_rank_batched(source, n_l, watched_bits, target_row, target_anime, content_batch(fit, batch),
                             "content_rank", fit["tok_offsets"].device)


def content_similar(fit, queries, k, keep=None, batch=CONTENT_BATCH):
    """The ``k`` nearest items of each query item by content: a query is a one-entry history of weight 1, so the score is
    the cosine of the two unit-length TF-IDF rows up to the 2^-30 quantisation of the profile; the query itself is never
    listed.  Returns (idx int32 [nq, k], score fp32 [nq, k]) in ``ops.rows_topk``'s order.  ValueError for a query
    outside the items."""
    q = np.asarray(_host(queries), np.int64).reshape(-1)
    n = int(fit["n_items"])
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("content_similar: query item out of range")
    own = np.zeros((q.size, (n + 31) // 32), np.uint32)
    own[np.arange(q.size), q >> 5] = np.uint32(1) << (q & 31).astype(np.uint32)
    bits = torch.as_tensor(own.view(np.int32), device=fit["tok_offsets"].device)
    return content_topk(fit, np.arange(q.size + 1), q.astype(np.int32), None, k, bits, keep, batch)


# ----------------------------------------------------------------------------------------
# implicit-feedback ALS: no model takes part
# ----------------------------------------------------------------------------------------
ALS_BATCH = 4096        # users per anirec_dot_scores call: a score row each


def _als_csr(row, col, n_rows, excess):
    """(offsets int64 [n_rows + 1], col int32, excess | None) on the device: a stable sort by ``row``, so a row's entries
    keep the pairs' own order"""
    order = torch.sort(row, stable=True)[1]
    off = torch.zeros(n_rows + 1, dtype=torch.int64, device=row.device)
    off[1:] = torch.cumsum(torch.bincount(row, minlength=n_rows), 0)
    return off, col[order].to(torch.int32).contiguous(), None if excess is None else excess[order].contiguous()


def als_fit(user_idx, item_idx, n_users, n_items, factors=64, sweeps=15, cg_steps=3, alpha=1.0, reg=0.01, weight=None,
            seed=0, device="cuda:0"):
    """Implicit-feedback matrix factorisation (Hu, Koren and Volinsky 2008) of the liked pairs (user_idx[t], item_idx[t]) by
    alternating least squares, every half-sweep ``cg_steps`` warm-started conjugate-gradient steps per row
    (``ops.als_half_sweep``).  A liked pair has preference 1 and confidence 1 + alpha * weight[t]
    (``weight`` None: 1), every other pair preference 0 and confidence 1; ``reg`` is the L2 weight on both tables.  A pair
    that repeats counts twice.  Both CSRs are built on the device; the start is
    ``default_rng(seed).standard_normal * 0.01`` in fp32, X then Y; a sweep is the user half then the item half, the Gram
    matrix recomputed before each (``ops.als_gram``).
    Returns {"X" fp32 [n_users, factors], "Y" fp32 [n_items, factors]} on the device, "loss" (the objective after every
    half-sweep: the row losses summed in fp64 + reg |frozen table|^2) and the parameters ("n_users", "n_items",
    "factors", "sweeps", "cg_steps", "alpha", "reg", "seed").  Raises ValueError, before any GPU use, for ``factors``
    outside the supported widths, ``cg_steps`` outside 0 .. 16, a negative ``sweeps``, ``alpha`` or ``reg``; and for an
    index out of range or a weight that is negative or not finite."""
    from . import ops
    factors, cg_steps, reg, alpha = ops.check_als(factors, cg_steps, reg, alpha)
    n_users, n_items, sweeps = int(n_users), int(n_items), int(sweeps)
    if n_users < 1 or n_items < 1 or sweeps < 0:
        raise ValueError("als_fit: n_users and n_items must be >= 1 and sweeps >= 0")
    u, i = _host(user_idx).reshape(-1), _host(item_idx).reshape(-1)
    if len(u) != len(i) or (weight is not None and len(_host(weight).reshape(-1)) != len(u)):
        raise ValueError("als_fit: user_idx, item_idx and weight must have one entry per pair")
    if len(u) and (u.min() < 0 or u.max() >= n_users or i.min() < 0 or i.max() >= n_items):
        raise ValueError("als_fit: index out of range")
    dev = torch.device(device)
    ud, idd = _on(u, dev, torch.int64), _on(i, dev, torch.int64)
    ex = None
    if weight is not None:
        w = _on(_host(weight).reshape(-1), dev, torch.float32)
        if w.numel() and not bool((torch.isfinite(w) & (w >= 0)).all()):
            raise ValueError("als_fit: weight must be finite and >= 0")
        ex = torch.tensor(alpha, dtype=torch.float32, device=dev) * w
    u_off, u_idx, u_ex = _als_csr(ud, idd, n_users, ex)
    i_off, i_idx, i_ex = _als_csr(idd, ud, n_items, ex)
    rng = np.random.default_rng(seed)
    X = torch.as_tensor((rng.standard_normal((n_users, factors)) * 0.01).astype(np.float32), device=dev)
    Y = torch.as_tensor((rng.standard_normal((n_items, factors)) * 0.01).astype(np.float32), device=dev)
    loss, flags = [], []
    for _ in range(sweeps):
        X, rl, e = ops.als_half_sweep(Y, ops.als_gram(Y), u_off, u_idx, X, reg, cg_steps, u_ex, alpha, check=False)
        loss.append(rl.double().sum() + reg * Y.double().square().sum())
        flags.append(e)
        Y, rl, e = ops.als_half_sweep(X, ops.als_gram(X), i_off, i_idx, Y, reg, cg_steps, i_ex, alpha, check=False)
        loss.append(rl.double().sum() + reg * X.double().square().sum())
        flags.append(e)
    if flags and int(torch.cat(flags).max().item()):
        raise ValueError("als_fit: index out of range")
    return {"X": X, "Y": Y, "loss": [float(v) for v in (torch.stack(loss).tolist() if loss else [])],
            "n_users": n_users, "n_items": n_items, "factors": factors, "sweeps": sweeps, "cg_steps": cg_steps,
            "alpha": alpha, "reg": reg, "seed": int(seed)}


def _als_users(fit, users):
    dev = fit["X"].device
    us = _on(_host(users).reshape(-1) if not isinstance(users, torch.Tensor) else users.reshape(-1), dev, torch.int64)
    if us.numel() and (int(us.min()) < 0 or int(us.max()) >= fit["X"].shape[0]):
        raise ValueError("als: user out of range")
    return us


def _als_source(fit, users):
    """(the row source of ``als_rows_source``, n_lists)"""
    from . import ops
    us = _als_users(fit, users)
    return lambda l0, l1: ops.dot_scores(fit["X"][us[l0:l1]], fit["Y"]), int(us.numel())


def als_topk(fit, users, k, watched_bits=None, batch=ALS_BATCH):
    """ALS recommendation lists: for each user of ``users`` (rows of ``fit["X"]``) the ``k`` best items by
    ``ops.dot_scores(X[users], Y)`` without a bit in ``watched_bits`` [n_listed, ceil(n_items/32)], taken by the exact
    select (``ops.rows_topk``), ``batch`` users at a time.  Returns (idx int32 [n_listed, k], score fp32 [n_listed, k])."""
    source, n_l = _als_source(fit, users)
    return rows_topk_batched(source, n_l, k, watched_bits, None, batch, "als_topk", fit["X"].device)


def als_rank(fit, users, watched_bits, target_row, target_anime, batch=ALS_BATCH):
    """The ranks ``ops.predict_rank`` gives a model, for the ALS scores of ``als_topk``: target t is (``target_row[t]``:
    a position in ``users``, ``target_anime[t]``); returns rank int32 [n_t] on the device (0 = first among the items the
    listed user has no watched bit for, the target's own bit ignored).  ``batch`` users at a time."""
    source, n_l = _als_source(fit, users)
    return rows_rank_batched(source, n_l, watched_bits, target_row, target_anime, batch, "als_rank", fit["X"].device)


# ----------------------------------------------------------------------------------------
# BPR matrix factorisation, the pairwise learned baseline (Rendle et al. 2009): no model takes part
# ----------------------------------------------------------------------------------------
PAIRWISE_SYSTEMS = ("bpr",)     # row-score systems beside HYBRID_SYSTEMS, CONTENT_SYSTEMS, ... (which stay as they are)
BPR_BATCH = ALS_BATCH           # users per anirec_dot_scores call: a score row each


def bpr_fit(user_idx, item_idx, n_users, n_items, factors=64, epochs=30, batch=131072, lr=0.05, reg=0.01, tries=8,
            bias=True, seed=0, device="cuda:0"):
    """BPR matrix factorisation (Rendle et al. 2009) of the liked pairs (user_idx[t], item_idx[t]) by mini-batch SGD on
    sampled (user, liked item, unliked item) triples (``ops.bpr_steps``).  A pair that repeats counts once.
    The start is ``default_rng(seed).standard_normal * 0.01`` in fp32, X then Y, as ``als_fit`` draws it; with ``bias`` the
    last column of X is then 1 and never written and that of Y starts at 0: an item bias, the scores still plain dot
    products.  An epoch is ``ceil(pairs / batch)`` steps of ``batch`` triples, drawn by a hash of (``seed``, step, slot);
    the negative is the first of ``tries`` hashed items the user has not liked.  The defaults are the literature's and the
    ``implicit`` library's common values, not tuned on this data.  The result is a function of the arguments alone, bit
    for bit.
    Returns {"X" fp32 [n_users, factors], "Y" fp32 [n_items, factors]} on the device, "counts" (per epoch: triples kept,
    slots dropped, kept triples already in the right order before their step), "n_pairs" and the parameters ("n_users",
    "n_items", "factors", "epochs", "batch", "lr", "reg", "tries", "bias", "seed").  Raises ValueError, before any GPU use,
    for ``factors`` outside the supported widths, a ``batch`` < 1, ``tries`` outside 1 .. 16, a negative ``epochs``, ``lr``
    or ``reg``, an index out of range, no pair at all or ``ceil(len(user_idx) / batch) * epochs`` of 2^31 or more; and,
    after the fit, for one that diverged (lower ``lr``)."""
    from . import ops
    factors, batch, tries, lr, reg, bias = ops.check_bpr(factors, batch, tries, lr, reg, bias)
    n_users, n_items, epochs = int(n_users), int(n_items), int(epochs)
    if n_users < 1 or n_items < 1 or epochs < 0:
        raise ValueError("bpr_fit: n_users and n_items must be >= 1 and epochs >= 0")
    u, i = _host(user_idx).reshape(-1), _host(item_idx).reshape(-1)
    if len(u) != len(i) or len(u) == 0:
        raise ValueError("bpr_fit: user_idx and item_idx must have one entry per pair, and one pair at least")
    if u.min() < 0 or u.max() >= n_users or i.min() < 0 or i.max() >= n_items:
        raise ValueError("bpr_fit: index out of range")
    if -(-len(u) // batch) * epochs >= 2 ** 31:       # on the pairs as given (no fewer than the distinct ones): no GPU yet
        raise ValueError("bpr_fit: ceil(pairs / batch) * epochs must stay below 2^31 steps")
    dev = torch.device(device)
    key = torch.unique(_on(u, dev, torch.int64) * n_items + _on(i, dev, torch.int64))       # sorted: rows, items ascending
    pair_user, idx = (key // n_items).to(torch.int32), (key % n_items).to(torch.int32)
    off = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(torch.bincount(pair_user.long(), minlength=n_users), 0)
    n_pairs = int(key.numel())
    rng = np.random.default_rng(seed)
    X0 = (rng.standard_normal((n_users, factors)) * 0.01).astype(np.float32)
    Y0 = (rng.standard_normal((n_items, factors)) * 0.01).astype(np.float32)
    if bias:
        X0[:, -1], Y0[:, -1] = 1.0, 0.0
    X, Y = torch.as_tensor(X0, device=dev), torch.as_tensor(Y0, device=dev)
    per = -(-n_pairs // batch)
    ws = torch.empty(ops.bpr_workspace_bytes(n_users, n_items, factors, batch), dtype=torch.uint8, device=dev)
    counts, flags = [], []
    for e in range(epochs):
        c, f = ops.bpr_steps(X, Y, off, idx, pair_user, batch, tries, seed, e * per, per, lr, reg, bias, workspace=ws,
                             check=False)
        counts.append(c.sum(0))
        flags.append(f)
    if flags:
        flag = 0
        for f in torch.cat(flags).tolist():
            flag |= int(f)
        ops.bpr_raise(flag, "bpr_fit")
    return {"X": X, "Y": Y, "counts": [[int(v) for v in row] for row in (torch.stack(counts).tolist() if counts else [])],
            "n_pairs": n_pairs, "n_users": n_users, "n_items": n_items, "factors": factors, "epochs": epochs,
            "batch": batch, "lr": lr, "reg": reg, "tries": tries, "bias": bool(bias), "seed": int(seed)}


def bpr_topk(fit, users, k, watched_bits=None, batch=BPR_BATCH):
    """BPR recommendation lists: ``als_topk`` on a ``bpr_fit``'s tables (``ops.dot_scores(X[users], Y)``, the exact select,
    ``batch`` users at a time).  Returns (idx int32 [n_listed, k], score fp32 [n_listed, k])."""
    source, n_l = _als_source(fit, users)
    return rows_topk_batched(source, n_l, k, watched_bits, None, batch, "bpr_topk", fit["X"].device)


def bpr_rank(fit, users, watched_bits, target_row, target_anime, batch=BPR_BATCH):
    """The ranks ``als_rank`` gives, for the scores of a ``bpr_fit``: rank int32 [n_t] on the device."""
    source, n_l = _als_source(fit, users)
    return rows_rank_batched(source, n_l, watched_bits, target_row, target_anime, batch, "bpr_rank", fit["X"].device)


def bpr_rows_source(fit, users):
    """A row source of the BPR scores of ``users`` (rows of ``fit["X"]``), through ``ops.dot_scores``."""
    return _als_source(fit, users)[0]


# ----------------------------------------------------------------------------------------
# EASE, the closed-form linear item-item autoencoder (Steck 2019): no model takes part
# ----------------------------------------------------------------------------------------
EASE_SYSTEMS = ("ease",)    # row-score systems beside HYBRID_SYSTEMS and CONTENT_SYSTEMS (which stay as they are)
EASE_BATCH = 4096           # users per anirec_ease_scores call: a score row each
EASE_REG = 500.0            # the paper's value for a data set of about this many users; not tuned on this data


def ease_fit(user_idx, anime_idx, rating, n_users, n_items, liked_min_rating=0.0, reg=EASE_REG, neighbours=0,
             device="cuda:0"):
    """An EASE model from a rating list: a user LIKED an anime when the (scaled) rating is at or above
    ``liked_min_rating`` (compared in fp32; 0.0 = every rating).  With B the 0/1 item x user matrix of liked pairs:
    G = B B^T (the exact count rows of ``ops.cooc_scores``, COOC_BATCH query items at a time), A = G + reg I in fp64,
    P = A^-1 (``ops.spd_inverse``), W = -P / diag(P) with a zero diagonal (``ops.ease_weights``).  ``reg`` = 500 is the
    paper's value for a data set of about this many users; it is not tuned on this data.  The inverse is held to its
    residual for reg >= 1; a reg far below 1 on a rank-deficient G is outside the tested domain.
    Returns {"W" fp32 [n_items, n_items], "pop" int32 [n_items] (how many users liked each anime)} on the device and the
    parameters ("reg", "n_items", "n_users", "n_liked", "liked_min_rating", "neighbours").  With ``neighbours`` = K > 0
    the fit additionally holds "knn": the K largest entries of every row of W other than the diagonal, as the
    {"nbr_idx", "nbr_sim"} tables of an item-kNN model (``ops.rows_topk`` with ``self_idx``); the rows of this
    truncated model are ``itemknn_rows_source(fit["knn"], ...)``.
    Raises ValueError, before any GPU use, for a ``reg`` that is not finite or not > 0 or a negative ``neighbours``;
    and, naming ``reg``, when the inverse meets a pivot that is not positive."""
    from . import ops
    reg, neighbours = ops.check_ease(reg, neighbours)
    n_users, n_items = int(n_users), int(n_items)
    if n_users < 1 or n_items < 1:
        raise ValueError("ease_fit: n_users and n_items must be >= 1")
    if neighbours > max(1, n_items - 1):
        raise ValueError("ease_fit: neighbours = %d is more than the %d other items" % (neighbours, n_items - 1))
    u, a = _host(user_idx).reshape(-1), _host(anime_idx).reshape(-1)
    r = _host(rating).reshape(-1).astype(np.float32)
    if not len(u) == len(a) == len(r):
        raise ValueError("ease_fit: user_idx, anime_idx and rating must have one entry per rating")
    liked = r >= np.float32(liked_min_rating)
    dev = torch.device(device)
    bits = item_bits(torch.as_tensor(u[liked].astype(np.int32), device=dev),
                     torch.as_tensor(a[liked].astype(np.int32), device=dev), n_users, n_items, device=dev)
    A = torch.empty(n_items, n_items, dtype=torch.float64, device=dev)
    q = torch.arange(n_items, dtype=torch.int32, device=dev)
    pop = None
    for q0 in range(0, n_items, COOC_BATCH):
        _, cnt, _, pp = ops.cooc_scores(bits, n_users, q[q0:q0 + COOC_BATCH], count=True, pop=pop is None)
        pop = pp if pop is None else pop
        A[q0:q0 + COOC_BATCH] = cnt
    A.diagonal().add_(reg)
    P, info = ops.spd_inverse(A)
    del A
    if int(info.item()):
        raise ValueError("ease_fit: the inverse met a pivot that is not positive in block step %d: reg = %r is too "
                         "small for this data" % (int(info.item()) - 1, reg))
    W = ops.ease_weights(P)
    del P
    fit = {"W": W, "pop": pop, "reg": reg, "n_items": n_items, "n_users": n_users, "n_liked": int(liked.sum()),
           "liked_min_rating": float(liked_min_rating), "neighbours": neighbours}
    if neighbours:
        idx = torch.empty(n_items, neighbours, dtype=torch.int32, device=dev)
        sim = torch.empty(n_items, neighbours, dtype=torch.float32, device=dev)
        for q0 in range(0, n_items, COOC_BATCH):
            idx[q0:q0 + COOC_BATCH], sim[q0:q0 + COOC_BATCH] = ops.rows_topk(W[q0:q0 + COOC_BATCH], neighbours,
                                                                             self_idx=q[q0:q0 + COOC_BATCH])
        fit["knn"] = {"nbr_idx": idx, "nbr_sim": sim}
    return fit


def _ease_source(fit, offsets, hist_idx, hist_w):
    """(the row source of ``ease_rows_source``, n_lists)"""
    from . import ops
    off = np.asarray(_host(offsets), np.int64).reshape(-1)
    if off.size < 1:
        raise ValueError("ease: offsets holds n_lists + 1 entries")
    dev = fit["W"].device
    hi = _on(hist_idx, dev, torch.int32)
    hw = None if hist_w is None else _on(hist_w, dev, torch.float32)
    return lambda l0, l1: ops.ease_scores(fit["W"], off[l0:l1 + 1], hi, hw), int(off.size) - 1


def ease_rows_source(fit, offsets, hist_idx, hist_w=None):
    """A row source of the EASE scores of the lists ``ease_topk`` takes, through ``ops.ease_scores``."""
    return _ease_source(fit, offsets, hist_idx, hist_w)[0]


def ease_topk(fit, offsets, hist_idx, hist_w=None, k=10, watched_bits=None, keep=None, batch=EASE_BATCH):
    """EASE recommendation lists: list l's history ``hist_idx[offsets[l]:offsets[l + 1]]`` (``history_csr`` builds it;
    ``hist_w`` None = weight 1) scored through the weights of ``fit`` (``ops.ease_scores``) and the ``k`` best anime
    without a bit in ``watched_bits`` [n_lists, ceil(n_items/32)] and with ``keep`` [n_items] set taken by the exact
    select (``ops.rows_topk``), ``batch`` lists at a time.  Returns (idx int32 [n_lists, k], score fp32 [n_lists, k])."""
    source, n_l = _ease_source(fit, offsets, hist_idx, hist_w)
    return rows_topk_batched(source, n_l, k, watched_bits, keep, batch, "ease_topk", fit["W"].device)


def ease_rank(fit, offsets, hist_idx, hist_w, watched_bits, target_row, target_anime, batch=EASE_BATCH):
    """The ranks ``ops.predict_rank`` gives a model, for the EASE scores of ``ease_topk``: target t is
    (``target_row[t]``: a list, ``target_anime[t]``); returns rank int32 [n_t] on the device (0 = first among the anime
    the list has no watched bit for, the target's own bit ignored).  ``batch`` lists at a time."""
    source, n_l = _ease_source(fit, offsets, hist_idx, hist_w)
    return rows_rank_batched(source, n_l, watched_bits, target_row, target_anime, batch, "ease_rank", fit["W"].device)


def ease_similar(fit, queries, k, keep=None, batch=EASE_BATCH):
    """The ``k`` anime with the largest weights in each query item's row of W (what liking the query adds most to); the
    query itself is never listed.  Returns (idx int32 [nq, k], score fp32 [nq, k]) in ``ops.rows_topk``'s order.
    ValueError for a query outside the items."""
    q = np.asarray(_host(queries), np.int64).reshape(-1)
    n = int(fit["n_items"])
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("ease_similar: query item out of range")
    own = np.zeros((q.size, (n + 31) // 32), np.uint32)
    own[np.arange(q.size), q >> 5] = np.uint32(1) << (q & 31).astype(np.uint32)
    dev = fit["W"].device
    qd = torch.as_tensor(q, device=dev)
    return rows_topk_batched(lambda l0, l1: fit["W"][qd[l0:l1]], int(q.size), k,
                             torch.as_tensor(own.view(np.int32), device=dev), keep, batch, "ease_similar", dev)


# ----------------------------------------------------------------------------------------
# RP3beta, the three-step random walk with a popularity penalty (Cooper et al. 2014, Paudel et al. 2017; DESIGN.md
# §4.25): no model takes part
# ----------------------------------------------------------------------------------------
GRAPH_SYSTEMS = ("rp3",)    # row-score systems beside HYBRID_SYSTEMS, CONTENT_SYSTEMS and EASE_SYSTEMS (which stay)
RP3_ALPHA = 1.0             # common values from the literature (alpha = 1, beta = 0 is the plain walk P3); not tuned
RP3_BETA = 0.3              # on this data
RP3_NEIGHBOURS = 100
RP3_MAX_Q = 16383           # ANIREC_WCOOC_MAX_Q: the user weight is an integer of 14 bits


def rp3_user_weights(deg, alpha):
    """The integer user weights of an RP3 fit, int32 [n_users], on the host in NumPy fp64: 0 where ``deg`` (how many
    items the user liked) is 0, else max(1, rint(16383 (d_min / deg) ** alpha)) with d_min the smallest positive degree.
    14 bits: the walk's deg ** -alpha relative to the lightest user's, so that every sum over users is one of integers.
    A user with 10 000 likes gets 2 instead of 1.6 when d_min is 1: the heaviest users are the coarsest."""
    deg = np.asarray(_host(deg), np.int64).reshape(-1)
    q = np.zeros(len(deg), np.int32)
    pos = deg > 0
    if pos.any():
        d_min = np.float64(deg[pos].min())
        q[pos] = np.maximum(1.0, np.rint(16383.0 * (d_min / deg[pos].astype(np.float64)) ** np.float64(alpha))) \
            .astype(np.int32)
    return q


def check_rp3(alpha, beta, neighbours):
    """(alpha, beta as floats, neighbours as an int), or a ValueError before any GPU use: an ``alpha`` or ``beta`` that
    is negative or not finite, a negative ``neighbours``."""
    alpha, beta, neighbours = float(alpha), float(beta), int(neighbours)
    for name, v in (("alpha", alpha), ("beta", beta)):
        if not (0.0 <= v < float("inf")):
            raise ValueError("rp3: %s = %r must be finite and >= 0" % (name, v))
    if neighbours < 0:
        raise ValueError("rp3: neighbours = %d must be >= 0" % neighbours)
    return alpha, beta, neighbours


def _rp3_pow2(m):
    """the power of two that puts ``m`` in [256, 512); 1 for an m that is not a positive number"""
    if not (m > 0.0 and m < float("inf")):
        return 1.0
    return float(np.ldexp(1.0, 9 - int(np.frexp(m)[1])))


def rp3_fit(user_idx, anime_idx, rating, n_users, n_items, liked_min_rating=0.0, alpha=RP3_ALPHA, beta=RP3_BETA,
            neighbours=RP3_NEIGHBOURS, device="cuda:0"):
    """An RP3beta model from a rating list: a user LIKED an anime when the (scaled) rating is at or above
    ``liked_min_rating`` (compared in fp32; 0.0 = every rating).  With pop(i) the users who liked item i and deg(u) the
    items user u liked:  W[i][j] = pop(i)^-alpha pop(j)^-beta sum_{u liked i and j} deg(u)^-alpha  off the diagonal, 0
    on it; a history H scores item j as sum_{i in H} h_i W[i][j].  alpha = 1, beta = 0 is the plain three-step walk P3,
    beta > 0 the popularity penalty.  The defaults (1.0, 0.3, 100 neighbours) are common values from the literature,
    not tuned on this data.  The user term is the integer ``rp3_user_weights`` (14 bits), the sum S over users is exact
    (``ops.wcooc_scores`` on the i8 matrix cores, COOC_BATCH query items a call), w = float32((float64(S) pop(i)^-alpha)
    pop(j)^-beta) with fp64 scale arrays from the host (0 where pop is 0).  Every row keeps its ``neighbours`` largest
    weights (``ops.rows_topk`` under the call's own excl rows: never the item itself nor an item without a common
    user) — truncation is part of the method; ``neighbours`` = 0 keeps the dense matrix.  All kept weights are then
    multiplied by the one power of two that puts the largest of them in [256, 512): exact, no ranking changes, and
    history weights up to 2 stay inside ``ops.itemknn_scores``' term bound of 1024.
    Returns {"nbr_idx" int32 [n_items, K], "nbr_sim" fp32 [n_items, K]} (the tables of an item-kNN model; padded with
    -1 / NaN) or, for neighbours = 0, {"W" fp32 [n_items, n_items]} with a zero diagonal; plus "pop" int32 [n_items],
    "deg" int32 [n_users], "user_q" int32 [n_users] on the device and the parameters ("alpha", "beta", "neighbours",
    "scale", "n_items", "n_users", "n_liked", "liked_min_rating").
    Raises ValueError, before any GPU use, for an ``alpha`` / ``beta`` that is negative or not finite, a negative
    ``neighbours`` or more than the other items, columns of unequal length."""
    from . import ops
    alpha, beta, neighbours = check_rp3(alpha, beta, neighbours)
    n_users, n_items = int(n_users), int(n_items)
    ops.check_wcooc(n_items, n_users)
    if neighbours > max(1, n_items - 1):
        raise ValueError("rp3_fit: neighbours = %d is more than the %d other items" % (neighbours, n_items - 1))
    u, a = _host(user_idx).reshape(-1), _host(anime_idx).reshape(-1)
    r = _host(rating).reshape(-1).astype(np.float32)
    if not len(u) == len(a) == len(r):
        raise ValueError("rp3_fit: user_idx, anime_idx and rating must have one entry per rating")
    liked = r >= np.float32(liked_min_rating)
    dev = torch.device(device)
    ud = torch.as_tensor(u[liked].astype(np.int32), device=dev)
    ad = torch.as_tensor(a[liked].astype(np.int32), device=dev)
    bits = item_bits(ud, ad, n_users, n_items, device=dev)
    # (the popcounts of the rows of both bit matrices: a repeated pair counts once, as in the bits)
    pop = ops.cooc_scores(bits, n_users, [0], pop=True)[3]
    deg = ops.cooc_scores(ops.seen_bits(ud, ad, n_users, n_items, device=dev), n_items, [0], pop=True)[3]
    del ud, ad
    user_q = rp3_user_weights(deg, alpha)
    p = _host(pop).astype(np.float64)
    row, col = np.zeros(n_items), np.zeros(n_items)
    row[p > 0] = p[p > 0] ** np.float64(-alpha)
    col[p > 0] = p[p > 0] ** np.float64(-beta)
    uq = torch.as_tensor(user_q, device=dev)
    row, col = torch.as_tensor(row, device=dev), torch.as_tensor(col, device=dev)
    q = torch.arange(n_items, dtype=torch.int32, device=dev)
    fit = {"pop": pop, "deg": deg, "user_q": uq, "alpha": alpha, "beta": beta, "neighbours": neighbours,
           "n_items": n_items, "n_users": n_users, "n_liked": int(liked.sum()),
           "liked_min_rating": float(liked_min_rating)}
    if neighbours:
        idx = torch.empty(n_items, neighbours, dtype=torch.int32, device=dev)
        sim = torch.empty(n_items, neighbours, dtype=torch.float32, device=dev)
        for q0 in range(0, n_items, COOC_BATCH):
            w, _, ex = ops.wcooc_scores(bits, n_users, uq, q[q0:q0 + COOC_BATCH], row, col, excl=True)
            idx[q0:q0 + COOC_BATCH], sim[q0:q0 + COOC_BATCH] = ops.rows_topk(w, neighbours, wbits=ex)
        kept = torch.where(idx >= 0, sim, torch.zeros_like(sim))
        fit["scale"] = _rp3_pow2(float(kept.max().item()))
        fit["nbr_idx"], fit["nbr_sim"] = idx, sim * fit["scale"]
    else:
        W = torch.empty(n_items, n_items, dtype=torch.float32, device=dev)
        for q0 in range(0, n_items, COOC_BATCH):
            W[q0:q0 + COOC_BATCH] = ops.wcooc_scores(bits, n_users, uq, q[q0:q0 + COOC_BATCH], row, col)[0]
        W.diagonal().zero_()
        fit["scale"] = _rp3_pow2(float(W.max().item()))
        fit["W"] = W.mul_(fit["scale"])
    return fit


def _rp3_source(fit, offsets, hist_idx, hist_w):
    """(the row source of ``rp3_rows_source``, n_lists)"""
    return _ease_source(fit, offsets, hist_idx, hist_w) if "W" in fit else _knn_source(fit, offsets, hist_idx, hist_w)


def _rp3_device(fit):
    return (fit["W"] if "W" in fit else fit["nbr_idx"]).device


def rp3_rows_source(fit, offsets, hist_idx, hist_w=None):
    """A row source of the RP3 scores of the lists ``rp3_topk`` takes: ``itemknn_rows_source`` over a truncated fit,
    ``ease_rows_source`` over a dense one (``ops.itemknn_scores`` / ``ops.ease_scores``: the same fixed-point sums)."""
    return _rp3_source(fit, offsets, hist_idx, hist_w)[0]


def rp3_topk(fit, offsets, hist_idx, hist_w=None, k=10, watched_bits=None, keep=None, batch=ITEMKNN_BATCH):
    """RP3 recommendation lists: list l's history ``hist_idx[offsets[l]:offsets[l + 1]]`` (``history_csr`` builds it;
    ``hist_w`` None = weight 1, at most 2) scored through the weights of ``fit`` and the ``k`` best anime without a bit
    in ``watched_bits`` [n_lists, ceil(n_items/32)] and with ``keep`` [n_items] set taken by the exact select
    (``ops.rows_topk``), ``batch`` lists at a time.  Returns (idx int32 [n_lists, k], score fp32 [n_lists, k])."""
    source, n_l = _rp3_source(fit, offsets, hist_idx, hist_w)
    return rows_topk_batched(source, n_l, k, watched_bits, keep, batch, "rp3_topk", _rp3_device(fit))


def rp3_rank(fit, offsets, hist_idx, hist_w, watched_bits, target_row, target_anime, batch=ITEMKNN_BATCH):
    """The ranks ``ops.predict_rank`` gives a model, for the RP3 scores of ``rp3_topk``: target t is
    (``target_row[t]``: a list, ``target_anime[t]``); returns rank int32 [n_t] on the device (0 = first among the anime
    the list has no watched bit for, the target's own bit ignored).  ``batch`` lists at a time."""
    source, n_l = _rp3_source(fit, offsets, hist_idx, hist_w)
    return rows_rank_batched(source, n_l, watched_bits, target_row, target_anime, batch, "rp3_rank", _rp3_device(fit))


def rp3_similar(fit, queries, k, keep=None, batch=ITEMKNN_BATCH):
    """The ``k`` anime with the largest weights in each query item's row of the fit (where a walk from the query ends
    most often): of the dense W, or of the row's kept neighbours; the query itself is never listed.  Returns (idx int32
    [nq, k], score fp32 [nq, k]) in ``ops.rows_topk``'s order.  ValueError for a query outside the items."""
    q = np.asarray(_host(queries), np.int64).reshape(-1)
    n = int(fit["n_items"])
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("rp3_similar: query item out of range")
    dev = _rp3_device(fit)
    qd = torch.as_tensor(q, device=dev)
    out = np.zeros((q.size, ((n + 31) // 32) * 32), bool)      # the anime that are no candidates of a row
    if "W" in fit:
        out[np.arange(q.size), q] = True
        source = lambda l0, l1: fit["W"][qd[l0:l1]]
    else:
        ni, ns = fit["nbr_idx"][qd].long(), fit["nbr_sim"][qd]
        nh = _host(ni)
        out[:, :n] = True
        rr, cc = np.nonzero(nh >= 0)
        out[rr, nh[rr, cc]] = False
        rows = torch.zeros(q.size, n + 1, dtype=torch.float32, device=dev)      # (column n takes the padding slots)
        rows.scatter_(1, torch.where(ni >= 0, ni, torch.full_like(ni, n)), ns)
        rows = rows[:, :n].contiguous()
        source = lambda l0, l1: rows[l0:l1]
    wb = (out.reshape(q.size, -1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return rows_topk_batched(source, int(q.size), k, torch.as_tensor(wb.view(np.int32), device=dev), keep, batch,
                             "rp3_similar", dev)


# ----------------------------------------------------------------------------------------
# hybrid lists: several systems' score rows fused into one
# ----------------------------------------------------------------------------------------
HYBRID_SYSTEMS =("model", "popularity", "itemknn", "als")
HYBRID_BATCH = 4096     # users per anirec_fuse_rows call: a score row per system and a fused row each


def check_hybrid(systems, weights=None, method="rrf", rrf_c=60):
    """(systems as a tuple of names, weights as floats, the method's name, rrf_c), or a ValueError before any GPU use:
    a name that is not one of HYBRID_SYSTEMS + CONTENT_SYSTEMS + EASE_SYSTEMS + GRAPH_SYSTEMS + PAIRWISE_SYSTEMS, a name
    twice, no name at all, and what ``ops.check_fuse`` refuses (a
    weights list of another length among it)."""
    from . import ops
    names = [systems] if isinstance(systems, str) else list(systems)
    names = [str(s).strip().lower() for s in names]
    known = HYBRID_SYSTEMS + CONTENT_SYSTEMS + EASE_SYSTEMS + GRAPH_SYSTEMS + PAIRWISE_SYSTEMS
    for s in names:
        if s not in known:
            raise ValueError("hybrid system %r is not one of %s" % (s, ", ".join(known)))
    if not names or len(set(names)) != len(names):
        raise ValueError("hybrid systems %r must be one or more distinct names of %s" % (names, ", ".join(known)))
    _, _, ws, _, rrf_c = ops.check_fuse(len(names), 1, weights, method, rrf_c)
    return tuple(names), ws, str(method).strip().lower(), rrf_c


def model_rows_source(U, A, head, users):
    """A row source (``(l0, l1) -> fp32 [l1 - l0, n_anime]``) of the model's predicted ratings of ``users`` (rows of
    ``U``), through ``ops.predict_grid``."""
    from . import ops
    us = np.asarray(_host(users), np.int64).reshape(-1)
    return lambda l0, l1: ops.predict_grid(U, A, head, us[l0:l1])


def itemknn_rows_source(knn, offsets, hist_idx, hist_w=None):
    """A row source of the item-kNN scores of the lists ``itemknn_topk`` takes, through ``ops.itemknn_scores``."""
    return _knn_source(knn, offsets, hist_idx, hist_w)[0]


def als_rows_source(fit, users):
    """A row source of the ALS scores of ``users`` (rows of ``fit["X"]``), through ``ops.dot_scores``."""
    return _als_source(fit, users)[0]


def hybrid_rows_source(sources, weights=None, method="rrf", rrf_c=60, watched_bits=None, keep=None):
    """A row source of the fused rows (``ops.fuse_rows`` over the member sources' rows of a span, under the span's
    ``watched_bits`` and ``keep``): a callable member is asked for its rows, a 1-D vector is shared by every list."""
    from . import ops
    sources = list(sources)
    return lambda l0, l1: ops.fuse_rows([src(l0, l1) if callable(src) else src for src in sources], weights, method,
                                        rrf_c, wbits=_span_bits(watched_bits, l0, l1), keep=keep)


def hybrid_topk(sources, k, weights=None, method="rrf", rrf_c=60, watched_bits=None, keep=None, batch=HYBRID_BATCH,
                n_lists=None):
    """Hybrid recommendation lists: ``sources`` one row source per system (a callable ``(l0, l1) -> fp32 [l1 - l0,
    n_anime]`` on the device: ``model_rows_source``, ``itemknn_rows_source``, ``als_rows_source``; or a 1-D vector shared
    by every list: ``popularity_scores``), fused per list by ``ops.fuse_rows`` under ``watched_bits`` [n_lists,
    ceil(n_anime/32)] and ``keep`` [n_anime], and the ``k`` best taken by the exact select (``ops.rows_topk``), ``batch``
    lists at a time.  ``n_lists`` defaults to the rows of ``watched_bits``.  Returns (idx int32 [n_lists, k], score fp32
    [n_lists, k]: the fused values) like ``als_topk``."""
    if n_lists is None:
        if watched_bits is None:
            raise ValueError("hybrid_topk: n_lists is needed without watched_bits")
        n_lists = int(watched_bits.shape[0])
    fused = hybrid_rows_source(sources, weights, method, rrf_c, watched_bits, keep)
    return rows_topk_batched(fused, n_lists, k, watched_bits, keep, batch, "hybrid_topk")


def hybrid_rank(sources, watched_bits, target_row, target_anime, weights=None, method="rrf", rrf_c=60,
                batch=HYBRID_BATCH):
    """The ranks ``ops.predict_rank`` gives a model, for the fused rows of ``hybrid_topk``: target t is
    (``target_row[t]``: a list, ``target_anime[t]``); returns rank int32 [n_t] on the device (0 = first among the anime
    the list has no watched bit for).  Raises ValueError if a target has its own watched bit set: a fused row holds no
    value there.  ``batch`` lists at a time."""
    if watched_bits is None:
        raise ValueError("hybrid_rank: watched_bits [n_lists, ceil(n_anime/32)] is needed")
    if not isinstance(watched_bits, torch.Tensor):
        watched_bits = torch.as_tensor(np.ascontiguousarray(watched_bits))
    fused = hybrid_rows_source(sources, weights, method, rrf_c, watched_bits)
    return rows_rank_batched(fused, int(watched_bits.shape[0]), watched_bits, target_row, target_anime, batch,
                             "hybrid_rank", own_bit_clear=True)


# learned hybrid weights: every target's rank under a grid of weight vectors, and the best vector
HYBRID_GRID_BATCH = 1024            # users per anirec_fuse_rank_grid call: a score row and a unit row per system each
HYBRID_GRID_WS_BYTES = 1 << 30      # the batch shrinks until the call's workspace fits in this
HYBRID_TUNE_METRICS = ("ndcg@K", "hit_rate@K", "mrr")


def hybrid_weight_grid(n_sys, steps):
    """The candidate weight vectors of a simplex grid, fp32 [n_w, n_sys]: row 0 all ones (the untuned default), then
    every integer composition (i_0 .. i_{S-1}) of ``steps`` in ascending lexicographic order as fl32(i_s / steps):
    n_w = 1 + C(steps + S - 1, S - 1).  ValueError for n_sys outside 1 .. 8, steps < 1, or more than 4095 rows
    (``ops.FUSE_MAX_GRID``)."""
    import math
    from . import ops
    n_sys, steps = int(n_sys), int(steps)
    if not 1 <= n_sys <= ops.FUSE_MAX_SYS:
        raise ValueError("hybrid_weight_grid: n_sys = %d must be in 1 .. %d" % (n_sys, ops.FUSE_MAX_SYS))
    if steps < 1:
        raise ValueError("hybrid_weight_grid: steps = %d must be >= 1" % steps)
    n_w = 1 + math.comb(steps + n_sys - 1, n_sys - 1)
    if n_w > ops.FUSE_MAX_GRID:
        raise ValueError("hybrid_weight_grid: steps = %d over %d systems gives %d weight vectors, more than the %d one "
                         "grid call ranks" % (steps, n_sys, n_w, ops.FUSE_MAX_GRID))
    grid = np.asarray(_compositions(steps, n_sys), np.float64) / float(steps)
    return np.concatenate([np.ones((1, n_sys), np.float32), grid.astype(np.float32)])


def _compositions(total, parts):
    """the tuples of ``parts`` non-negative integers with sum ``total``, in ascending lexicographic order"""
    if parts == 1:
        return [(total,)]
    return [(i,) + rest for i in range(total + 1) for rest in _compositions(total - i, parts - 1)]


def hybrid_rank_grid(sources, watched_bits, target_row, target_anime, weight_grid, method="rrf", rrf_c=60,
                     batch=HYBRID_GRID_BATCH):
    """``hybrid_rank`` under every weight vector of ``weight_grid`` [n_w, n_sys] at once (``ops.fuse_rank_grid``):
    returns rank int32 [n_w, n_t] on the device, row w what ``hybrid_rank(..., weights=weight_grid[w])`` returns.  The
    span loop of ``rows_rank_batched``: ``batch`` lists at a time (fewer where the call's workspace would pass
    HYBRID_GRID_WS_BYTES), a span that holds no target is not scored, and no rank depends on the batch.  ValueError
    before any GPU use as ``ops.check_fuse_grid`` and ``hybrid_rank``."""
    from . import ops
    if watched_bits is None:
        raise ValueError("hybrid_rank_grid: watched_bits [n_lists, ceil(n_anime/32)] is needed")
    if not isinstance(watched_bits, torch.Tensor):
        watched_bits = torch.as_tensor(np.ascontiguousarray(watched_bits))
    sources = list(sources)
    n_lists = int(watched_bits.shape[0])
    _, _, grid, _, rrf_c = ops.check_fuse_grid(len(sources), 1, weight_grid, method, rrf_c)
    m_name = str(method).strip().lower()
    # a row's units take n_sys * 4 bytes an item; 32 items a watched word is an upper bound that needs no scoring
    per_row = len(sources) * 32 * max(1, int(watched_bits.shape[1])) * 4
    spans = _spans(n_lists, min(int(batch), max(1, HYBRID_GRID_WS_BYTES // per_row)), "hybrid_rank_grid")
    tr, ta = _targets("hybrid_rank_grid", target_row, target_anime, n_lists, watched_bits)
    rank = None
    for l0, l1 in spans:
        sel = np.flatnonzero((tr >= l0) & (tr < l1))
        if not sel.size:
            continue
        rows = [src(l0, l1) if callable(src) else src for src in sources]
        r = ops.fuse_rank_grid(rows, grid, m_name, rrf_c, tr[sel] - l0, ta[sel], wbits=_span_bits(watched_bits, l0, l1))
        if rank is None:
            rank = torch.empty(int(grid.shape[0]), int(tr.size), dtype=torch.int32, device=r.device)
        rank[:, torch.as_tensor(sel, device=rank.device)] = r
    return torch.empty(int(grid.shape[0]), 0, dtype=torch.int32) if rank is None else rank


def hybrid_tune_metric(metric):
    """(name, k or None) of a tuning metric: ``ndcg@K`` / ``hit_rate@K`` with an integer K >= 1, or ``mrr``; ValueError
    for anything else."""
    name = str(metric).strip().lower()
    if name == "mrr":
        return name, None
    head, _, k = name.partition("@")
    if head in ("ndcg", "hit_rate") and k.isdigit() and int(k) >= 1:
        return "%s@%d" % (head, int(k)), int(k)
    raise ValueError("hybrid tuning metric %r is not one of %s" % (metric, ", ".join(HYBRID_TUNE_METRICS)))


def hybrid_fit_weights(rank_grid, target_unit, n_units, metric, n_rows, units=None):
    """Which weight vector of a grid ranks a set of units' targets best: ``rank_grid`` int32 [n_w, n_t] on the device
    (``hybrid_rank_grid``), ``target_unit`` [n_t] each target's unit among ``n_units``, ``metric`` one of ndcg@K,
    hit_rate@K, mrr, ``n_rows`` the length of the gain table (the number of anime).  The per-unit gain sums are the exact
    int64 sums of ``ops.rank_gain_rows`` over ``rank_gain_tables``' fixed-point gains.  Returns (sums int64 NumPy
    [n_units, n_w], best): ``best`` the index of the largest total over ``units`` (an index array or a bool mask; None:
    every unit), ties to the lowest index, so that row 0 — equal weights — wins unless a vector is strictly better.
    Integer sums: the choice does not depend on the order of anything."""
    from . import ops
    name, k = hybrid_tune_metric(metric)
    tables, names, _ = rank_gain_tables([k if k is not None else 1], n_rows)
    gain = tables[names.index(name)][None, :]
    rows = ops.rank_gain_rows(rank_grid, target_unit, n_units, torch.as_tensor(gain.astype(np.int64)))
    sums = np.asarray(_host(rows), np.int64)[:, :-1]
    return sums, hybrid_best_weights(sums, units)


def hybrid_fold_deal(n_units, folds, seed):
    """int64 [n_units]: the fold of every unit, ``np.random.default_rng(seed).permutation(n_units) % folds``; ValueError
    for folds < 2"""
    folds = int(folds)
    if folds < 2:
        raise ValueError("hybrid tuning needs folds >= 2 (got %d): a fold's weights come from the other folds" % folds)
    return np.random.default_rng(int(seed)).permutation(int(n_units)).astype(np.int64) % folds


def hybrid_cross_fit(sums, fold, folds):
    """[folds] grid indices: entry f is ``hybrid_best_weights`` over the units that are NOT in fold f, so no unit helps
    choose the weights its own targets are ranked with"""
    fold = np.asarray(fold, np.int64)
    return [hybrid_best_weights(sums, fold != f) for f in range(int(folds))]


def hybrid_best_weights(sums, units=None):
    """the grid index with the largest total of ``sums`` [n_units, n_w] over ``units``; ties to the lowest index"""
    s = np.asarray(sums, np.int64)
    total = (s if units is None else s[np.asarray(units)]).sum(axis=0)
    return int(np.argmax(total))


# ----------------------------------------------------------------------------------------
# confidence intervals: a Poisson bootstrap over users
# ----------------------------------------------------------------------------------------
# floor(2**32 * CDF(j)) of Poisson(1), j = 0 .. 12 (from 60-digit decimals): the weight of a unit is the number of
# thresholds its hash reaches, 0 .. 13
POISSON1_THRESHOLDS = (0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c,
                       0xffffed1f, 0xfffffe21, 0xffffffd4, 0xfffffffc, 0xffffffff)
GAIN_SCALE = float(1 << 30)     # the fixed point of a gain table: q = rint(gain * 2**30)


def rank_gain_tables(ks, n_rows):
    """``ranking_metrics``' gains as integer tables over the ranks 0 .. n_rows - 1 (``ops.rank_gain_rows``): returns
    (tables uint32 [M, n_rows], names, scales float64 [M]) with the metrics ``hit_rate@k`` (rank < k) and ``ndcg@k``
    (1 / log2(rank + 2) where rank < k) for each k of ``ks`` in ascending order, then ``mrr`` (1 / (rank + 1)) and
    ``mean_rank`` (the rank itself).  A table holds rint(gain * 2**30) computed in float64, the mean-rank table the rank
    at scale 1: a metric is sum(table[rank]) / (scale * n), off from the float64 mean by at most 2**-31 per term.
    ValueError for no k, a k < 1 or n_rows < 1."""
    ks = sorted({int(k) for k in ks})
    n_rows = int(n_rows)
    if not ks or ks[0] < 1:
        raise ValueError("rank_gain_tables: at least one k >= 1 (got %r)" % (ks,))
    if not 1 <= n_rows < 1 << 31:
        raise ValueError("rank_gain_tables: n_rows must be in 1 .. 2**31 - 1")
    r = np.arange(n_rows, dtype=np.float64)
    dcg = 1.0 / np.log2(r + 2.0)
    tables = [np.where(r < k, 1.0, 0.0) for k in ks] + [np.where(r < k, dcg, 0.0) for k in ks] + [1.0 / (r + 1.0)]
    q = [np.rint(t * GAIN_SCALE).astype(np.uint32) for t in tables] + [np.arange(n_rows, dtype=np.uint32)]
    names = ["hit_rate@%d" % k for k in ks] + ["ndcg@%d" % k for k in ks] + ["mrr", "mean_rank"]
    scales = np.asarray([GAIN_SCALE] * (len(names) - 1) + [1.0], np.float64)
    return np.stack(q), names, scales


def check_bootstrap(n_rep, level):
    """``bootstrap_metrics``' checks of the replicate count and the level: (int n_rep >= 0, float level in (0, 1)), or a
    ValueError."""
    n_rep, level = int(n_rep), float(level)
    if n_rep < 0:
        raise ValueError("bootstrap: n_rep must be >= 0 (got %d)" % n_rep)
    if not 0.0 < level < 1.0:
        raise ValueError("bootstrap: level must lie inside (0, 1) (got %r)" % level)
    return n_rep, level


def bootstrap_figures(sums, scales, level=0.95):
    """The host part of the bootstrap, float64: ``sums`` int64 [B + 1, n_sys * M + 1] as ``ops.boot_sums`` returns them
    from ``ops.rank_gain_rows``' rows (row 0 the sample, row b replicate b; the last column the weighted number of
    targets), ``scales`` [M] the metrics' fixed points.  The figure of row b is sum / (scale * count).  Returns a dict
    of arrays: value [n_sys, M] (row 0), se (std with ddof = 1 of the replicates), lo / hi (np.quantile of the
    replicates at (1 - level) / 2 and (1 + level) / 2); for the systems after the first, on the same weights, diff
    [n_sys - 1, M] = first - other of the values, diff_lo / diff_hi the quantiles of the replicates' differences and
    p = min(1, 2 (1 + min(#{d <= 0}, #{d >= 0})) / (n_rep_used + 1)), two-sided; n_rep = B and n_rep_used, the replicates
    whose weighted count is above 0 (the others are dropped).  With fewer than 2 left, se, the quantiles and p are NaN."""
    _, level = check_bootstrap(0, level)
    s = np.asarray(sums, np.int64)
    scales = np.asarray(scales, np.float64).reshape(-1)
    M = int(scales.size)
    if s.ndim != 2 or s.shape[0] < 1 or M < 1 or (s.shape[1] - 1) % M or s.shape[1] - 1 < M:
        raise ValueError("bootstrap_figures: sums must be [B + 1, n_sys * %d + 1] (got %s)" % (M, tuple(s.shape)))
    n_sys = (s.shape[1] - 1) // M
    count = s[:, -1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fig = s[:, :-1].astype(np.float64).reshape(-1, n_sys, M) / (scales[None, None, :] * count[:, None, None])
    value = np.where(count[0] > 0, fig[0], np.nan)
    reps = fig[1:][s[1:, -1] > 0]
    used = int(reps.shape[0])
    d = reps[:, :1, :] - reps[:, 1:, :]
    nan = np.full((n_sys, M), np.nan)
    out = {"value": value, "se": nan, "lo": nan, "hi": nan, "diff": value[:1] - value[1:],
           "diff_lo": nan[1:], "diff_hi": nan[1:], "p": nan[1:], "n_rep": int(s.shape[0]) - 1, "n_rep_used": used}
    if used >= 2:
        qs = [(1.0 - level) / 2.0, (1.0 + level) / 2.0]
        out["se"] = reps.std(axis=0, ddof=1)
        out["lo"], out["hi"] = np.quantile(reps, qs, axis=0)
        out["diff_lo"], out["diff_hi"] = np.quantile(d, qs, axis=0) if n_sys > 1 else (nan[1:], nan[1:])
        tail = np.minimum((d <= 0).sum(axis=0), (d >= 0).sum(axis=0)).astype(np.float64)
        out["p"] = np.minimum(1.0, 2.0 * (1.0 + tail) / (used + 1.0))
    return out


def bootstrap_metrics(ranks_by_system, target_row, n_units, ks, n_rep=1000, seed=0, level=0.95, unit_key=None,
                      n_rows=None, device="cuda:0"):
    """Ranking metrics with their spread: a Poisson bootstrap over USERS — replicate b >= 1 re-weights
    every unit (a user: its held-out ratings are not independent) by an integer Poisson(1) draw that is a hash of
    (seed, b, the unit's key) and is never stored; replicate 0 is the sample itself.  ``ranks_by_system``: an ordered
    dict name -> ranks [n_t] (tensors on one device, or arrays; 0 = ranked first, a rank < 0 or >= ``n_rows`` gains
    nothing) of the same targets; the first system is the one the others are compared with.  ``target_row`` [n_t]: each
    target's position among the ``n_units`` units; ``unit_key`` [n_units]: the units' own numbers (the user indices;
    default 0 .. n_units - 1) — the weights follow the key, so a subset of the users re-draws the same weights.
    ``n_rows``: the length of the gain tables (default: the largest rank + 1).  The ranks are reduced to per-unit integer
    sums (``ops.rank_gain_rows``), those to replicate sums (``ops.boot_sums``), and ``bootstrap_figures`` reads them.
    Returns {"metrics": the names of ``rank_gain_tables(ks, n_rows)``, "systems", "n" (targets), "n_units", "n_rep",
    "n_rep_used", "level", "seed", "figures": {system: {metric: {"value", "se", "lo", "hi"}}}, "diffs": {other system:
    {metric: {"diff", "lo", "hi", "p"}}}} in float64.  ValueError before any GPU use for n_rep < 0, a level outside
    (0, 1), rank vectors of different lengths, no system, or a k < 1."""
    from . import ops
    n_rep, level = check_bootstrap(n_rep, level)
    ks = sorted({int(k) for k in ks})
    if not ks or ks[0] < 1:
        raise ValueError("bootstrap_metrics: at least one k >= 1 (got %r)" % (ks,))
    systems = list(ranks_by_system)
    if not systems:
        raise ValueError("bootstrap_metrics: at least one system")
    ranks = [ranks_by_system[s] for s in systems]
    n_units = int(n_units)
    n_t = int(np.asarray(_host(target_row)).size) if not isinstance(target_row, torch.Tensor) else int(target_row.numel())
    if any(int(r.numel() if isinstance(r, torch.Tensor) else np.asarray(r).size) != n_t for r in ranks):
        raise ValueError("bootstrap_metrics: every system must rank the same %d targets" % n_t)
    if unit_key is not None and int(np.asarray(_host(unit_key)).size) != n_units:
        raise ValueError("bootstrap_metrics: unit_key must hold one key per unit")
    dev = next((r.device for r in ranks if isinstance(r, torch.Tensor)), torch.device(device))
    if n_rows is None:
        n_rows = max([1] + [int(torch.as_tensor(r).max()) + 1 for r in ranks if n_t])
    tables, names, scales = rank_gain_tables(ks, n_rows)
    if n_t:
        rk = torch.stack([torch.as_tensor(_host(r) if not isinstance(r, torch.Tensor) else r, device=dev)
                          .reshape(-1).to(torch.int32) for r in ranks])
        rows = ops.rank_gain_rows(rk, torch.as_tensor(_host(target_row) if not isinstance(target_row, torch.Tensor)
                                                      else target_row, device=dev).reshape(-1).to(torch.int32),
                                  n_units, torch.as_tensor(tables.astype(np.int64), device=dev))
        key = np.arange(n_units, dtype=np.int64) if unit_key is None else np.asarray(_host(unit_key)).reshape(-1)
        key = torch.as_tensor((key.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32), device=dev)
        sums = _host(ops.boot_sums(rows, key, seed, n_rep, POISSON1_THRESHOLDS))
    else:
        sums = np.zeros((n_rep + 1, len(systems) * len(names) + 1), np.int64)
    f = bootstrap_figures(sums, scales, level)
    out = {"metrics": names, "systems": systems, "n": int(sums[0, -1]), "n_units": n_units, "n_rep": n_rep,
           "n_rep_used": f["n_rep_used"], "level": level, "seed": int(seed), "figures": {}, "diffs": {}}
    for i, s in enumerate(systems):
        out["figures"][s] = {m: {k: float(f[k][i, j]) for k in ("value", "se", "lo", "hi")} for j, m in enumerate(names)}
        if i:
            out["diffs"][s] = {m: {"diff": float(f["diff"][i - 1, j]), "lo": float(f["diff_lo"][i - 1, j]),
                                   "hi": float(f["diff_hi"][i - 1, j]), "p": float(f["p"][i - 1, j])}
                               for j, m in enumerate(names)}
    return out


# ----------------------------------------------------------------------------------------
# onboarding lists: a greedy maximum-coverage questionnaire: no model takes part
# ----------------------------------------------------------------------------------------
ONBOARD_STRATEGIES = ("coverage", "popularity")


def _user_words(users, n_users):
    """int32 [ceil(n_users/32)] with the bits of ``users`` set: the ``open_bits`` of ``ops.cover_greedy``."""
    flags = np.zeros(((n_users + 31) // 32) * 32, np.uint8)
    flags[np.asarray(users, np.int64)] = 1
    return np.packbits(flags.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).view(np.int32)


def _known_summary(level, users, depth):
    """Of ``users``: the share that knows >= 1 listed item, the share that knows >= ``depth``, the mean number known."""
    if len(users) == 0:
        return {"users": 0, "share_any": None, "share_depth": None, "mean_known": None}
    lv = level[users]
    return {"users": int(len(users)), "share_any": float((lv >= 1).mean()), "share_depth": float((lv >= depth).mean()),
            "mean_known": float(lv.mean())}


def onboarding_split(n_users, population=None, holdout=0.0, seed=0):
    """The (pick users, held-out users) of an onboarding list, both sorted: the population (None: every user; a bool mask
    [n_users]; or user indices) in ascending order, permuted by ``numpy.random.default_rng(seed).permutation`` on the
    host; the first ``floor(holdout * |population|)`` of the permutation are held out, the rest pick.  A function of
    ``n_users``, the population, ``holdout`` and ``seed`` alone."""
    n_users = int(n_users)
    holdout = float(holdout)
    if not 0.0 <= holdout < 1.0:
        raise ValueError("onboarding: holdout = %r must be in [0, 1)" % holdout)
    if population is None:
        pop = np.arange(n_users, dtype=np.int64)
    else:
        p = _host(population).reshape(-1)
        if p.dtype == np.bool_:
            if len(p) != n_users:
                raise ValueError("onboarding: a population mask holds one entry per user")
            pop = np.flatnonzero(p).astype(np.int64)
        else:
            pop = np.unique(p.astype(np.int64))
            if len(pop) and (pop[0] < 0 or pop[-1] >= n_users):
                raise ValueError("onboarding: population user out of range")
    perm = np.random.default_rng(int(seed)).permutation(len(pop))
    n_hold = int(np.floor(holdout * len(pop)))
    return np.sort(pop[perm[n_hold:]]), np.sort(pop[perm[:n_hold]])


def onboarding_list(user_idx, anime_idx, n_users, n_anime, m, depth=3, strategy="coverage", population=None, keep=None,
                    holdout=0.0, seed=0, device="cuda:0", bits=None):
    """Which ``m`` anime to show a newcomer: the greedy maximum-coverage list of the rated-by bits of
    the rating list (``item_bits``; or ``bits`` when the caller holds them).  The population's users (``population``:
    None = everyone, a bool mask or user indices) are split into pick and held-out users by ``onboarding_split``: a
    fixed ``numpy.random.default_rng(seed)`` permutation of the sorted population on the host, its first
    ``floor(holdout * |population|)`` entries held out.  ``strategy="coverage"``: each pick is the anime (``keep[i] != 0``)
    the most pick users with fewer than ``depth`` listed anime so far have rated (``ops.cover_greedy``);
    ``"popularity"``: the same call at depth = m, the most rated anime among the pick users.  The list is then scored on
    every user (``ops.cover_levels``).  Returns a dict of host values: ``pick`` int32 [m] (-1 padded), ``gain`` int32
    [m], ``rated_by`` int32 [m] (raters of the pick among ALL users), ``picks`` (made), ``greedy_depth``, and for
    ``pick_users`` and ``holdout_users`` each {"users", "share_any" (know >= 1), "share_depth" (know >= ``depth``),
    "mean_known"} (None where the group is empty)."""
    from . import ops
    strategy = str(strategy).strip().lower()
    if strategy not in ONBOARD_STRATEGIES:
        raise ValueError("onboarding strategy %r is not one of %s" % (strategy, ", ".join(ONBOARD_STRATEGIES)))
    m, depth = int(m), int(depth)
    ops.check_cover(m, depth)
    n_users, n_anime = int(n_users), int(n_anime)
    pick_users, held_users = onboarding_split(n_users, population, holdout, seed)
    if bits is None:
        bits = item_bits(user_idx, anime_idx, n_users, n_anime, device=device)
    greedy_depth = depth if strategy == "coverage" else m
    pick, gain, info = ops.cover_greedy(bits, n_users, m, greedy_depth, open_bits=_user_words(pick_users, n_users),
                                        keep=keep)
    level = _host(ops.cover_levels(bits, n_users, pick)).astype(np.int64)
    pop = _host(ops.cooc_scores(bits, n_users, [0], pop=True)[3]).astype(np.int32)     # the raters of every anime
    pick, gain, info = _host(pick).astype(np.int32), _host(gain).astype(np.int32), _host(info)
    rated = np.where(pick >= 0, pop[np.maximum(pick, 0)], 0).astype(np.int32)
    return {"strategy": strategy, "m": m, "depth": depth, "greedy_depth": int(greedy_depth), "pick": pick, "gain": gain,
            "rated_by": rated, "picks": int(info[0]), "pick_users": _known_summary(level, pick_users, depth),
            "holdout_users": _known_summary(level, held_users, depth)}
