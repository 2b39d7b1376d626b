"""Loader and comparison rules for tests/golden/ref_fn/recs.* (written by tests/golden/make_recs_fixtures.py from the
reference's own anime_recs, recommendations, get_df, main_df_by_anime and get_anime_df).

Ranked lists are compared as far as the reference defines them: it sorts with an unstable quicksort, so inside a tie
group (a run of fixture fp64 scores closer together than the comparison's bar)
only the set is defined.  Outside tie groups the order is exact; a group cut by the count may be represented by any
of its members."""
import io
import json
import os

import numpy as np
import pandas as pd

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fn")
SIM_BAR = 2e-6          # similarity vs the fp64 cosine of the reference's normalised rows
PRED_BAR = 1e-5         # prediction vs the float64 model (BASELINE.json's bar)
ALL = 100000            # the "every row" count
# reference output column -> metadata_by_index column
META_COL = {"Japanese name": "japanese_name"}


def load():
    """recs.json (settings, deviations) with the lists, column values and CSV inputs of recs.npz put back in place."""
    with open(os.path.join(HERE, "recs.json"), encoding="utf-8") as f:
        rec = json.load(f)
    z = np.load(os.path.join(HERE, "recs.npz"))
    rec["npz"] = {k: z[k] for k in z.files}
    lists = json.loads(z["lists_json"].tobytes().decode("utf-8"))
    for part in ("similar_anime", "model_recs"):
        for case, l in zip(rec[part]["cases"], lists[part]):
            case.update(l)
        rec[part]["rows"] = lists[part + "_rows"]
    rec["get_anime_df"].update(lists["get_anime_df"])
    return rec


def csv(rec, name):
    """One of the CSV inputs ("anime_csv", "synopses_csv") as a file object for pandas."""
    return io.BytesIO(rec["npz"][name].tobytes())


def ratings(rec, prefix="ratings"):
    z = rec["npz"]
    return pd.DataFrame({"user_id": z[prefix + "_user_id"], "anime_id": z[prefix + "_anime_id"],
                         "rating": z[prefix + "_rating"]})


def is_null(v):
    return v is None or (isinstance(v, float) and np.isnan(v))


def same_value(a, b):
    if is_null(a) or is_null(b):
        return is_null(a) and is_null(b)
    if isinstance(a, np.generic):
        a = a.item()
    return a == b


def full_case(cases, case, keys):
    """The count = every-row case of the same setting (its list holds every row the setting can return)."""
    return next(c for c in cases if c["count" if "count" in c else "n_recs"] == ALL
                and all(c[k] == case[k] for k in keys))


def groups(scores, bar):
    """Tie-group id of each position of a reference-ordered fp64 list (NaN scores form one group)."""
    out, gid = [], 0
    for i, v in enumerate(scores):
        if i:
            p = scores[i - 1]
            tied = (is_null(p) and is_null(v)) or (not is_null(p) and not is_null(v) and abs(p - v) < bar)
            gid += 0 if tied else 1
        out.append(gid)
    return out


def check_ranked(got_keys, got_scores, want_keys, full_keys, full_scores, bar, got_index=None):
    """got_* : the build's list; want_keys: the reference's list at this count; full_*: the reference's every-row list
    and its fp64 scores.  got_index: the build's row index of each listed key (for its own tie rule)."""
    got_keys = [int(k) for k in got_keys]
    assert len(got_keys) == len(want_keys), (len(got_keys), len(want_keys))
    assert len(set(got_keys)) == len(got_keys)
    gid = dict(zip(full_keys, groups(full_scores, bar)))
    s64 = dict(zip(full_keys, full_scores))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got_keys, want_keys)) if gid.get(g) != gid[w]]
    assert not bad, "order/set differs from the reference at (position, got, want) %s" % bad[:8]
    for k, s in zip(got_keys, np.asarray(got_scores, np.float64)):
        want = s64[k]
        if is_null(want):
            assert np.isnan(s), (k, s)
        else:
            assert abs(s - want) <= bar, (k, s, want)
    if got_index is not None:                      # the build's tie rule: equal fp32 scores by index, NaN last
        s = np.asarray(got_scores, np.float32)
        nan = np.isnan(s)
        assert not (nan[:-1] & ~nan[1:]).any(), "a NaN score before a number"
        idx = np.asarray(got_index)
        for i in range(len(s) - 1):
            if (s[i] == s[i + 1]) or (nan[i] and nan[i + 1]):
                assert idx[i] < idx[i + 1], (i, s[i], idx[i], idx[i + 1])


def expected_columns(rec, part, key):
    """The reference's non-score values of the listed row `key` (int), by column name."""
    rows = rec[part]["rows"]
    return dict(zip(rows["columns"], rows["data"][str(int(key))]))
