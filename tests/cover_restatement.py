"""NumPy restatement of the onboarding calls (include/anirec.h: anirec_cover_greedy, anirec_cover_levels): the rule of the
header comment, step for step.  A plain helper module, imported by the tests the way ``cooc_restatement`` is; the
``ops_*`` functions at the end have the signatures of the ``ops`` wrappers on NumPy arrays, for the CPU tests that run
the host logic without a device.

    bits     uint32 [n_items, ceil(n_users/32)]; bit u & 31 of word u >> 5; bits at positions >= n_users ignored
    P        every user, or the users whose bit of open_bits is set
    open     u in P and level_u < depth
    gain     #{open u : bit u of the row}; the pick is the candidate (keep, not picked) of the largest gain, ties to the
             lowest index; no candidate or a largest gain of 0 stops the list (-1 / 0 from there on)
    info     {picks made, #{u in P : level_u == depth}, |P|, 0}
"""
import numpy as np

from cooc_restatement import pack_bits, unpack_bits  # noqa: F401  (the same bit rows)

MAX_PICKS = 1024


def cover_greedy(bits, n_users, m, depth=1, open_bits=None, keep=None):
    """Returns (pick int32 [m], gain int32 [m], info int32 [4], level int64 [n_users])."""
    B = unpack_bits(bits, n_users)
    n = B.shape[0]
    P = np.ones(n_users, bool) if open_bits is None else unpack_bits(np.asarray(open_bits).reshape(1, -1), n_users)[0]
    cand = np.ones(n, bool) if keep is None else np.asarray(keep).reshape(-1)[:n] != 0
    cand = cand.copy()
    level = np.zeros(n_users, np.int64)
    pick = np.full(m, -1, np.int32)
    gain = np.zeros(m, np.int32)
    made = 0
    Bf = B.astype(np.float64)                                    # 0 / 1: sums below 2**53 are exact in float64 (and fast)
    for p in range(m):
        is_open = P & (level < depth)
        g = (Bf @ is_open.astype(np.float64)).astype(np.int64)
        g = np.where(cand, g, -1)
        i = int(np.argmax(g)) if n else -1                       # argmax: the first of the largest, the lowest index
        if i < 0 or g[i] <= 0:
            break
        pick[p], gain[p] = i, g[i]
        level[is_open & B[i]] += 1
        cand[i] = False
        made += 1
    info = np.array([made, int((P & (level == depth)).sum()), int(P.sum()), 0], np.int32)
    return pick, gain, info, level


def cover_levels(bits, n_users, picks):
    """Returns (level int32 [n_users], err)."""
    B = unpack_bits(bits, n_users)
    n = B.shape[0]
    level = np.zeros(n_users, np.int32)
    err = 0
    for t in np.asarray(picks, np.int64).reshape(-1):
        if t == -1:
            continue
        if not 0 <= t < n:
            err = 1
            continue
        level += B[int(t)]
    return level, err


# ---- the wrappers' signatures on NumPy arrays (tests that run host logic with ``ops`` replaced) ----------------------
def ops_cover_greedy(bits, n_users, m, depth=1, open_bits=None, keep=None):
    return cover_greedy(np.ascontiguousarray(bits).view(np.uint32), int(n_users), int(m), int(depth),
                        None if open_bits is None else np.ascontiguousarray(open_bits).view(np.uint32), keep)[:3]


def ops_cover_levels(bits, n_users, picks):
    level, err = cover_levels(np.ascontiguousarray(bits).view(np.uint32), int(n_users), picks)
    if err:
        raise ValueError("cover_levels: pick out of range")
    return level
