"""CPU tests of the mapped tables: the NumPy restatement of include/anirec.h's exact t-SNE on cases
worked by hand, its accuracy against a plain fp64 t-SNE, the affinity builder's host logic, ``recs.map_place`` on a hand
case, the binding and every refusal that needs no device, the embedding_map component's flag surface, and the three
planted cases (5-nearest-neighbour purity on the map exactly 1.0).

The fixed-point bound (test_fixed_point_sums_stay_within_the_derived_bound), u = 2^-24 the fp32 unit roundoff, first
order in u with one u of head-room for the higher orders:
    dx               one rounding of an exact difference: u
    dx*dx            2u + u = 3u;   d2 = xx + yy: 3u + u = 4u;   1 + d2: 4u + u = 5u;   q = 1 / (.): 6u
    w = q*q          12u + u = 13u; w*dx: 13u + u + u = 15u, on a value of at most 3 sqrt(3)/16 < 0.33
    a = val*q        6u + u = 7u;   a*dx: 7u + u + u = 9u, on a value of at most 1
    I(p)             rint(p * 2^30) / 2^30 is within 2^-31 of p
so a row's repulsive sum of n - 1 terms is within (n - 1) (0.33 * 16u + 2^-31) of the exact one, its attractive sum of m
stored terms within m (10u + 2^-31), and Z within n (n - 1) (7u + 2^-31).  The fp64 yardstick's own float sums err by
n * 2^-53 a row: nothing beside these.
"""
import ctypes
import os

import numpy as np
import pytest

import tsne_restatement as R
from anime_recommendations_amd import _lib, build, ops, recs
from component_cli import load_component

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
S = 2 ** 30
U = 2.0 ** -24


def _scalar_forces(Y, P):
    """the header's chain pair by pair in Python: np.float32 scalars, Python ints (P dense, P' units)"""
    n = len(Y)
    Rx, Ry, Ax, Ay, Z = [0] * n, [0] * n, [0] * n, [0] * n, 0
    q30 = lambda p: int(np.rint(F32(p) * F32(S)))  # noqa: E731
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            dx, dy = F32(Y[i][0]) - F32(Y[j][0]), F32(Y[i][1]) - F32(Y[j][1])
            d2 = F32(F32(dx * dx) + F32(dy * dy))
            q = F32(1) / F32(F32(1) + d2)
            w = F32(q * q)
            Z += q30(q)
            Rx[i] += q30(F32(w * dx))
            Ry[i] += q30(F32(w * dy))
            if P[i][j]:
                a = F32(F32(P[i][j]) * q)
                Ax[i] += q30(F32(a * dx))
                Ay[i] += q30(F32(a * dy))
    return Rx, Ry, Ax, Ay, Z


def _forces(Y, P):
    Y = np.asarray(Y, F32)
    return R.forces(Y, *R.csr_from_dense(np.asarray(P, F32)))


# ---- the restatement on cases worked by hand ----------------------------------------------------------------------------
def test_two_points_by_hand():
    # (0,0) and (1,0): d2 = 1, q = 1/2, w = 1/4; stored P' = 1 both ways: a = 1/2
    Rx, Ry, Ax, Ay, Z, info = _forces([[0, 0], [1, 0]], [[0, 1], [1, 0]])
    assert Z == 2 * 2 ** 29 and info == 0
    assert Rx.tolist() == [-2 ** 28, 2 ** 28] and Ry.tolist() == [0, 0]
    assert Ax.tolist() == [-2 ** 29, 2 ** 29] and Ay.tolist() == [0, 0]
    # the update: n = 2, e = 1: att = -2^29 / (2^31 * 2) = -1/8, rep = -2^28 / 2^30 = -1/4, grad = 4 (-1/8 + 1/4) = 1/2;
    # v = 0 so the signs differ: g = 1.2; v = 0.8 * 0 - (10 * 1.2) * 0.5 = -6
    Y, V, G = R.update(np.array([[0, 0], [1, 0]], F32), np.zeros((2, 2)), np.ones((2, 2)), Rx, Ry, Ax, Ay, Z, 1.0, 0.8, 10.0)
    assert V.tolist() == [[-6.0, 0.0], [6.0, 0.0]] and Y.tolist() == [[-6.0, 0.0], [7.0, 0.0]]
    # (the y coordinate: grad = 0 and v = 0 have EQUAL signs, so the gain shrinks)
    assert G.tolist() == [[1.2, 0.8], [1.2, 0.8]]
    # exaggerated: att = 12 * -1/8 = -3/2, grad = 4 (-3/2 + 1/4) = -5, momentum 0.5: v = +60
    Y, V, G = R.update(np.array([[0, 0], [1, 0]], F32), np.zeros((2, 2)), np.ones((2, 2)), Rx, Ry, Ax, Ay, Z, 12.0, 0.5, 10.0)
    assert V[:, 0].tolist() == [60.0, -60.0]


def test_three_points_by_hand_and_the_scalar_chain():
    Y = [[0, 0], [1, 0], [0, 2]]                    # d2 = 1, 4, 5: q = 1/2, fl(1/5), fl(1/6)
    P = [[0, 0.5, 0], [0.5, 0, 1.25], [0, 1.25, 0]]
    Rx, Ry, Ax, Ay, Z, info = _forces(Y, P)
    q5, q6 = F32(1) / F32(5), F32(1) / F32(6)
    assert Z == 2 * (2 ** 29 + int(np.rint(q5 * F32(S))) + int(np.rint(q6 * F32(S))))
    assert Rx[0] == -2 ** 28 and Ry[0] == int(np.rint(F32(q5 * q5) * F32(-2) * F32(S)))
    assert Ax[0] == -2 ** 28 and Ay[0] == 0 and Ax[2] == int(np.rint(F32(F32(1.25) * q6) * F32(-1) * F32(S)))
    sRx, sRy, sAx, sAy, sZ = _scalar_forces(Y, P)
    assert (Rx.tolist(), Ry.tolist(), Ax.tolist(), Ay.tolist(), Z) == (sRx, sRy, sAx, sAy, sZ)
    rng = np.random.default_rng(3)                  # and on 40 random points with a random symmetric graph
    Y = (rng.standard_normal((40, 2)) * 3).astype(F32)
    P = np.triu((rng.random((40, 40)) < 0.2) * rng.random((40, 40)) * 2, 1)
    P = (P + P.T).astype(F32)
    Rx, Ry, Ax, Ay, Z, info = _forces(Y, P)
    assert (Rx.tolist(), Ry.tolist(), Ax.tolist(), Ay.tolist(), Z) == _scalar_forces(Y, P) and info == 0
    # fl(a - b) = -fl(b - a): the sums over all rows cancel pair by pair
    assert sum(Rx.tolist()) == 0 and sum(Ry.tolist()) == 0 and sum(Ax.tolist()) == 0


def test_a_duplicate_pair_counts_in_z_and_exerts_no_force():
    Rx, Ry, Ax, Ay, Z, info = _forces([[3, 4], [3, 4]], [[0, 2], [2, 0]])
    assert Z == 2 * S and not Rx.any() and not Ry.any() and not Ax.any() and not Ay.any() and info == 0
    Rx, Ry, Ax, Ay, Z3, info = _forces([[3, 4], [3, 4], [4, 4]], np.zeros((3, 3)))
    assert Z3 == 2 * S + 4 * 2 ** 29 and Rx.tolist() == [-2 ** 28, -2 ** 28, 2 ** 29]


def test_an_isolated_row_is_only_repelled_and_a_far_table_has_z_zero():
    P = [[0, 1, 0], [1, 0, 0], [0, 0, 0]]
    Rx, Ry, Ax, Ay, Z, info = _forces([[0, 0], [1, 0], [0, 1]], P)
    assert Ax[2] == 0 and Ay[2] == 0 and Ry[2] > 0 and Ax[0] < 0 and info == 0
    far = np.array([[0, 0], [50000, 0], [0, 50000]], F32)      # 50000 > 2^15.5: q * 2^30 < 1/2
    Rx, Ry, Ax, Ay, Z, info = _forces(far, P)
    assert Z == 0 and not Rx.any() and not Ry.any() and info == 0
    Y, V, G = R.update(far, np.zeros((3, 2)), np.ones((3, 2)), Rx, Ry, Ax, Ay, Z, 1.0, 0.8, 10.0)
    assert np.isfinite(Y).all() and V[2].tolist() == [0.0, 0.0]             # Z = 0: the repulsive term is 0


def test_rows_that_are_out_and_bad_stored_pairs_contribute_nothing():
    Y = np.array([[0, 0], [1, 0], [np.nan, 0], [0, np.inf], [0, 2.0 ** 61], [0, 1]], F32)
    P = np.zeros((6, 6), F32)
    P[0, 1] = P[1, 0] = P[0, 2] = P[2, 0] = P[5, 3] = P[3, 5] = 1
    got = _forces(Y, P)
    keep = [0, 1, 5]
    want = _forces(Y[keep], P[np.ix_(keep, keep)])
    assert got[5] == 1 and want[5] == 0 and got[4] == want[4]
    for g, w in zip(got[:4], want[:4]):
        assert g[keep].tolist() == w.tolist() and not g[[2, 3, 4]].any()
    off, idx, val = R.csr_from_dense(np.array([[0, 1], [1, 0]], F32))
    Y2 = np.array([[0, 0], [1, 0]], F32)
    r = R.forces(Y2, off, idx, np.array([3.0, 1.0], F32))
    assert r[5] == 2 and r[2].tolist() == [0, 2 ** 29]                      # a value above 2
    r = R.forces(Y2, off, idx, np.array([np.nan, 1.0], F32))
    assert r[5] == 2 and r[2].tolist() == [0, 2 ** 29]
    r = R.forces(Y2, off, np.array([7, 0], np.int32), val)
    assert r[5] == 4 and r[2].tolist() == [0, 2 ** 29]                      # an index outside the table
    r = R.forces(Y2, off, np.array([0, 0], np.int32), val)
    assert r[5] == 4 and r[2].tolist() == [0, 2 ** 29]                      # a stored self pair
    r = R.forces(Y2, np.array([0, 3, 2], np.int64), idx, val)
    assert r[5] == 4 and not r[2].any()                                     # offsets that are no lists


def test_the_term_bounds_at_the_distances_that_maximise_them():
    # |w dx| is largest at d = 1/sqrt(3): 3 sqrt(3)/16; |a dx| at d = 1 with P' = 2: 1; q at d = 0: 1
    d = F32(1 / np.sqrt(3))
    Rx, _, Ax, _, Z, _ = _forces([[0, 0], [d, 0]], [[0, 2], [2, 0]])
    assert abs(Rx[1] / S - 3 * np.sqrt(3) / 16) < 16 * U and Rx[1] < 0.33 * S
    for dd in np.linspace(0.3, 0.9, 601):
        assert abs(_forces([[0, 0], [F32(dd), 0]], np.zeros((2, 2)))[0][1]) <= Rx[1] + 1
    Rx, _, Ax, _, Z, _ = _forces([[0, 0], [1, 0]], [[0, 2], [2, 0]])
    assert Ax.tolist() == [-S, S] and abs(int(Ax[1])) < 2 ** 31
    for dd in np.linspace(0.7, 1.3, 601):
        assert abs(_forces([[0, 0], [F32(dd), 0]], [[0, 2], [2, 0]])[2][1]) <= S
    assert _forces([[5, 5], [5, 5]], np.zeros((2, 2)))[4] == 2 * S
    # the largest usable coordinate: d2 = 2^121 and 2^122, finite, every term 0
    big = _forces([[2.0 ** 60, 2.0 ** 60], [-2.0 ** 60, -2.0 ** 60]], [[0, 2], [2, 0]])
    assert big[4] == 0 and big[5] == 0 and not big[0].any() and not big[2].any()
    # a row sum stays inside int64 for n < 2^31: 2^31 terms of at most 2^30 (Z, the n^2 sum, does not: two words)
    assert (2 ** 31) * S < 2 ** 63 and (2 ** 20) ** 2 * S > 2 ** 63
    assert R.z_words(5 * 2 ** 64 + 7).tolist() == [7, 5]


# ---- accuracy: the fp64 yardstick -----------------------------------------------------------------------------------
def _case(n=120, seed=4):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 8))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    off, idx, val = R.dense_affinities(X, 12.0)
    Y = (rng.standard_normal((n, 2)) * 2).astype(F32)
    return off, idx, val, Y, R.dense_P(off, idx, val, n)


def test_the_fp64_gradient_is_the_derivative_of_kl():
    off, idx, val, Y, P = _case(40)
    Y = Y.astype(np.float64)
    g = R.grad_fp64(Y, P)
    h = 1e-5
    for i, c in ((0, 0), (7, 1), (39, 0)):
        Yp, Ym = Y.copy(), Y.copy()
        Yp[i, c] += h
        Ym[i, c] -= h
        fd = (R.kl_fp64(Yp, P) - R.kl_fp64(Ym, P)) / (2 * h)
        assert abs(fd - g[i, c]) < 1e-8 + 1e-6 * abs(g[i, c])


def test_fixed_point_sums_stay_within_the_derived_bound():
    for n, seed in ((120, 4), (333, 5)):
        off, idx, val, Y, P = _case(n, seed)
        Rx, Ry, Ax, Ay, Z, info = R.forces(Y, off, idx, val)
        Rf, Af, Zf = R.sums_fp64(Y, P * (2.0 * n))                          # (P' units, as the integer sums are)
        bound_r = (n - 1) * (0.33 * 16 * U + 2.0 ** -31)
        bound_a = np.diff(off).max() * (10 * U + 2.0 ** -31)
        bound_z = n * (n - 1) * (7 * U + 2.0 ** -31)
        fixed_r = np.stack([Rx, Ry], 1) / S
        fixed_a = np.stack([Ax, Ay], 1) / S
        err_r, err_a, err_z = np.abs(fixed_r - Rf).max(), np.abs(fixed_a - Af).max(), abs(Z / S - Zf)
        print("n %d: R %.3e of %.3e, A %.3e of %.3e, Z %.3e of %.3e" % (n, err_r, bound_r, err_a, bound_a, err_z, bound_z))
        assert err_r <= bound_r and err_a <= bound_a and err_z <= bound_z and info == 0
        assert np.abs(Rf).max() > 1000 * bound_r                             # the bound says something


# ---- the affinities on the host ---------------------------------------------------------------------------------------
def test_bisection_reaches_the_perplexity_within_the_bracket():
    rng = np.random.default_rng(6)
    d2 = rng.random((200, 90)) * 2
    d2[3] = 0.5                                     # every neighbour equally far: uniform at any beta
    for perp in (5.0, 30.0, 89.0):
        p, beta = R.conditional_p(d2, perp)
        assert np.allclose(p.sum(axis=1), 1.0, atol=1e-12) and (p > 0).all()
        got = R.row_perplexity(p)
        # 64 halvings of a bracket that opened at a power of two: beta is within 2^-52 relative of the root, and the
        # perplexity's sensitivity d log(perp) / d log(beta) is at most log(k)^2 / 4 < 6
        ok = np.ones(200, bool)
        ok[3] = False
        assert np.abs(got[ok] / perp - 1).max() < 6 * 2.0 ** -50
        assert abs(got[3] - 90) < 1e-9
    import torch
    pt, bt = recs._map_bandwidths(torch.as_tensor(d2), 30.0)
    p, beta = R.conditional_p(d2, 30.0)
    assert np.abs(pt.numpy() - p).max() < 1e-12 and np.abs(bt.numpy() / beta - 1).max() < 1e-12
    # symmetrised: P'_ij = p(j|i) + p(i|j), every stored pair both ways, rows ascending
    nbr = np.argsort(rng.random((200, 199)), axis=1)[:, :90]
    nbr = nbr + (nbr >= np.arange(200)[:, None])                            # skip the row itself
    off, idx, val = R.symmetrise(nbr, p)
    D = np.zeros((200, 200))
    D[np.arange(200)[:, None], nbr] = p
    want = R.csr_from_dense((D + D.T).astype(F32))
    assert np.array_equal(off, want[0]) and np.array_equal(idx, want[1]) and np.array_equal(val, want[2])
    assert abs(val.sum() / 400 - 1) < 1e-6 and val.max() <= 2
    to, ti, tv = recs._map_symmetrise(torch.as_tensor(nbr), pt, 200)
    assert np.array_equal(to.numpy(), off) and np.array_equal(ti.numpy(), idx) and np.abs(tv.numpy() - val).max() < 1e-7
    assert abs(recs.map_kl(torch.zeros(200, 2), to, ti, tv) - R.kl_fp64(np.zeros((200, 2)), R.dense_P(off, idx, val, 200))) < 1e-9


def test_map_place_on_a_hand_case():
    import torch
    Y = torch.tensor([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0], [9.0, 9.0]])
    nbr = torch.tensor([[0, 1], [2, 0]])
    cos = torch.tensor([[0.9, 0.9], [0.99, 0.5]])
    got = recs._map_place_positions(Y, nbr, cos, 2.0).numpy()
    assert got[0].tolist() == [1.0, 0.0]            # equally near two rows: halfway between them
    p, _ = R.conditional_p(2.0 - 2.0 * cos.numpy().astype(np.float64), 2.0)
    assert np.allclose(p, 0.5)                      # perplexity 2 over 2 neighbours is the uniform weight
    got = recs._map_place_positions(Y, nbr, cos, 1.2).numpy()
    p, _ = R.conditional_p(2.0 - 2.0 * cos.numpy().astype(np.float64), 1.2)
    assert p[1, 0] > 0.9 and np.allclose(got[1], [0.0, 2.0 * p[1, 0]], atol=1e-6) and got[1, 1] > 1.8
    assert recs.map_lr(17560) == 17560 / 48 and recs.map_lr(150) == 50.0


# ---- the binding and the refusals --------------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported():
    P = _lib.PROTOTYPES
    assert len(P["anirec_tsne_tile"][1]) == 0 and P["anirec_tsne_tile"][0] is ctypes.c_size_t
    assert len(P["anirec_tsne_workspace_bytes"][1]) == 2 and P["anirec_tsne_workspace_bytes"][0] is ctypes.c_size_t
    assert len(P["anirec_tsne_forces"][1]) == 14 and P["anirec_tsne_forces"][0] is ctypes.c_int
    assert len(P["anirec_tsne_fit"][1]) == 17 and P["anirec_tsne_fit"][0] is ctypes.c_int
    assert _lib.ABI_VERSION == 5 and "anirec_tsne.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "anirec.h")).read()
    for name in ("anirec_tsne_tile", "anirec_tsne_workspace_bytes", "anirec_tsne_forces", "anirec_tsne_fit"):
        assert name + "(" in header
    assert "#define ANIREC_TSNE_MAX_ROWS %d" % _lib.TSNE_MAX_ROWS in header and _lib.TSNE_MAX_ROWS >= 2 ** 20
    assert "#define ANIREC_TSNE_MAX_ITER %d" % _lib.TSNE_MAX_ITER in header and "#define ANIREC_ABI_VERSION 5" in header
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.anirec_abi_version() == 5 and lib.anirec_tsne_tile() == _lib.TSNE_TILE
    assert lib.anirec_tsne_workspace_bytes(100, 7) >= 100 * 24 + 7 * 16
    for bad in ((0, 7), (-1, 7), (_lib.TSNE_MAX_ROWS + 1, 7), (100, 0), (100, _lib.TSNE_MAX_ITER + 1)):
        assert lib.anirec_tsne_workspace_bytes(*bad) == 0
    assert lib.anirec_tsne_workspace_bytes(_lib.TSNE_MAX_ROWS, _lib.TSNE_MAX_ITER) > 0


def test_entry_points_refuse_bad_arguments_without_a_device():
    build.build(verbose=False)
    lib = _lib.load()
    fake = 4096         # never followed: every refusal comes before anything is enqueued
    D = ctypes.c_double

    def forces(n=50, nnz=10, j_splits=0, **null):
        p = {k: (None if null.get(k) else fake) for k in ("Y", "off", "idx", "val", "rx", "ry", "ax", "ay", "z", "info")}
        return lib.anirec_tsne_forces(p["Y"], n, p["off"], p["idx"], p["val"], nnz, j_splits, p["rx"], p["ry"], p["ax"],
                                      p["ay"], p["z"], p["info"], None)

    def fit(n=50, nnz=10, iters=5, exag=2, e=12.0, lr=50.0, j_splits=0, ws=fake, ws_bytes=None, **null):
        p = {k: (None if null.get(k) else fake) for k in ("Y", "off", "idx", "val", "V", "G", "info")}
        need = lib.anirec_tsne_workspace_bytes(50, 5) if ws_bytes is None else ws_bytes
        return lib.anirec_tsne_fit(p["Y"], n, p["off"], p["idx"], p["val"], nnz, iters, exag, D(e), D(lr), j_splits,
                                   p["V"], p["G"], p["info"], ws, need, None)

    for kw in (dict(n=0), dict(n=-3), dict(n=_lib.TSNE_MAX_ROWS + 1), dict(nnz=-1), dict(j_splits=-1),
               dict(j_splits=_lib.TSNE_MAX_SPLITS + 1)):
        assert forces(**kw) == -1, kw
        assert fit(**kw) == -1, kw
    for kw in (dict(iters=0), dict(iters=-1), dict(iters=_lib.TSNE_MAX_ITER + 1), dict(exag=-1), dict(e=0.0), dict(e=-1.0),
               dict(e=float("nan")), dict(e=float("inf")), dict(lr=0.0), dict(lr=float("nan")), dict(lr=float("inf")),
               dict(ws=None), dict(ws=fake + 4), dict(ws_bytes=0), dict(iters=6)):
        assert fit(**kw) == -1, kw
    assert fit(ws_bytes=lib.anirec_tsne_workspace_bytes(50, 5) - 1) == -1
    assert fit(n=51) == -1                                      # a workspace sized for 50 rows is too small for 51
    for name in ("Y", "off", "idx", "val", "rx", "ry", "ax", "ay", "z", "info"):
        assert forces(**{name: True}) == -1, name
    for name in ("Y", "off", "idx", "val", "V", "G", "info"):
        assert fit(**{name: True}) == -1, name


def test_ops_and_recs_refusals_need_no_gpu():
    import torch
    assert ops.check_tsne(100, 1000, 250, 12.0, 50.0, 3) == (100, 1000, 250, 12.0, 50.0, 3)
    for kw, msg in ((dict(n_rows=0), "n_rows = 0"), (dict(n_rows=_lib.TSNE_MAX_ROWS + 1), "TSNE_MAX_ROWS"),
                    (dict(iters=0), "iters = 0"), (dict(iters=4097), r"1 \.\. 4096"), (dict(exag_iters=-1), "exag_iters"),
                    (dict(exaggeration=0.0), "exaggeration"), (dict(exaggeration=float("nan")), "exaggeration"),
                    (dict(lr=-1.0), "lr = "), (dict(lr=float("inf")), "lr = "), (dict(j_splits=-1), "j_splits"),
                    (dict(j_splits=1025), "j_splits")):
        with pytest.raises(ValueError, match=msg):
            ops.check_tsne(**dict(dict(n_rows=100), **kw))
    Y = torch.zeros(4, 2)
    off, idx, val = torch.tensor([0, 1, 2, 2, 2]), torch.tensor([1, 0]), torch.tensor([1.0, 1.0])
    with pytest.raises(ValueError, match=r"\[n_rows, 2\]"):
        ops.tsne_forces(torch.zeros(4, 3), off, idx, val)
    with pytest.raises(ValueError, match="offsets must rise"):
        ops.tsne_forces(Y, torch.tensor([0, 2, 1, 2, 2]), idx, val)
    with pytest.raises(ValueError, match="offsets must rise"):
        ops.tsne_fit(Y, off[:-1], idx, val, 5)
    with pytest.raises(ValueError, match="one entry per stored pair"):
        ops.tsne_fit(Y, off, idx, val[:1], 5)
    with pytest.raises(ValueError, match="iters = 0"):
        ops.tsne_fit(Y, off, idx, val, 0)
    with pytest.raises(ValueError, match="n_rows = 0"):
        ops.tsne_forces(Y[:0], off[:1], idx[:0], val[:0])
    W = np.random.default_rng(0).normal(size=(9, 32)).astype(np.float32)
    for kw, msg in ((dict(perplexity=0.5), "perplexity"), (dict(neighbours=9), r"1 \.\. 8"), (dict(neighbours=0), "neighbours"),
                    (dict(perplexity=30.0), "cannot exceed the 8 neighbours"), (dict(perplexity=5.0, neighbours=4), "cannot exceed")):
        with pytest.raises(ValueError, match=msg):
            recs.map_affinities(W, **kw)
    with pytest.raises(ValueError, match="2 .. "):
        recs.map_affinities(W[:1], 1.0)
    with pytest.raises(ValueError, match="embedding_size"):
        recs.map_affinities(W[:, :20], 2.0)
    with pytest.raises(ValueError, match="iters = 5000"):
        recs.map_rows(W, 2.0, iters=5000)
    with pytest.raises(ValueError, match=r"init must be \[9, 2\]"):
        recs.map_rows(W, 2.0, init=np.zeros((8, 2)))
    assert recs.check_map(17560, 30.0) == (30.0, 90) and recs.check_map(50, 30.0) == (30.0, 49)


# ---- the component's flag surface --------------------------------------------------------------------------------------
def test_embedding_map_parser_and_mlproject_agree():
    mod = load_component("embedding_map")
    from anime_recommendations_amd import components as C
    assert mod.STR_FLAGS == ["main_df", "main_df_type", "project_name", "anime_df", "anime_df_type", "model", "model_type",
                             "map_fn", "map_type"] and mod.BOOL_FLAGS == ["save_map"]
    assert mod.OPTIONAL_FLAGS == {"map_table": "anime", "map_perplexity": 30.0, "map_iters": 1000, "map_seed": 0,
                                  "map_max_rows": 50000, "map_clusters": 0, "map_query": None, "map_plot": True}
    parser = mod.make_parser()
    argv = []
    for f in mod.STR_FLAGS:
        argv += ["--" + f, "x"]
    argv += ["--save_map", "True"]
    ns = parser.parse_args(argv)
    assert {f: getattr(ns, f) for f in mod.OPTIONAL_FLAGS} == mod.OPTIONAL_FLAGS and ns.save_map is True
    assert sorted(vars(ns)) == sorted(mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS))
    ns = parser.parse_args(argv + ["--map_table", " User", "--map_perplexity", "12.5", "--map_iters", "4096", "--map_seed", "7",
                                   "--map_max_rows", "0", "--map_clusters", "20", "--map_query", "Cowboy Bebop",
                                   "--map_plot", "false"])
    assert (ns.map_table, ns.map_perplexity, ns.map_iters, ns.map_seed, ns.map_max_rows, ns.map_clusters, ns.map_query,
            ns.map_plot) == ("user", 12.5, 4096, 7, 0, 20, "Cowboy Bebop", False)
    assert parser.parse_args(argv + ["--map_query", "none"]).map_query is None
    for bad in (["--map_table", "genre"], ["--map_perplexity", "0.5"], ["--map_perplexity", "nan"], ["--map_perplexity", "x"],
                ["--map_iters", "0"], ["--map_iters", "4097"], ["--map_seed", "-1"], ["--map_max_rows", "-1"],
                ["--map_clusters", "-1"], ["--map_clusters", "4097"], ["--map_plot", "maybe"], ["--save_map", "maybe"]):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + bad)
    with pytest.raises(ValueError, match="anime, user"):
        mod.map_table("genre")
    with pytest.raises(ValueError, match="1 .. 4096"):
        mod.map_iters("0")
    import yaml
    ml = yaml.safe_load(open(os.path.join(ROOT, "embedding_map", "MLproject")))
    assert ml["name"] == "embedding_map" and ml["conda_env"] == "conda.yml" and list(ml["entry_points"]) == ["main"]
    main = ml["entry_points"]["main"]
    params = main["parameters"]
    assert list(params) == mod.STR_FLAGS + mod.BOOL_FLAGS + list(mod.OPTIONAL_FLAGS)
    assert all(v["description"] for v in params.values()) and all(v["type"] == "str" for v in params.values())
    for f, v in params.items():                                 # the MLproject defaults parse to the parser's own
        assert ("default" in v) == (f in mod.OPTIONAL_FLAGS)
        if "default" in v:
            assert getattr(mod, f)(v["default"]) == mod.OPTIONAL_FLAGS[f]
    assert main["command"] == "python embedding_map.py " + " ".join("--%s {%s}" % (f, f) for f in params)
    assert yaml.safe_load(open(os.path.join(ROOT, "embedding_map", "conda.yml")))["name"] == "embedding_map"
    # the sample and the frame on the host
    assert C.map_sample(10, 0, 3).tolist() == list(range(10)) and C.map_sample(10, 10, 3).tolist() == list(range(10))
    take = C.map_sample(1000, 50, 3, always=999)
    assert len(take) == 50 and len(set(take.tolist())) == 50 and 999 in take and (np.diff(take) > 0).all()
    assert np.array_equal(take, C.map_sample(1000, 50, 3, always=999)) and not np.array_equal(take, C.map_sample(1000, 50, 4))
    import pandas as pd
    import torch
    fit = {"Y": torch.tensor([[0.0, 0.0], [1.0, 0.0], [float("nan"), float("nan")], [0.0, 3.0]])}
    frame = C.map_frame(fit, "anime", [10, 11, 12, 13], pd.DataFrame({"Name": ["a", "b", np.nan, "d"]}))
    assert frame.columns.tolist() == ["anime_id", "name", "x", "y", "cluster"] and frame["name"].tolist() == ["a", "b", "12", "d"]
    assert frame["cluster"].tolist() == [-1] * 4 and np.isnan(frame["x"][2])
    assert C.map_neighbours_on_map(frame, 0, 5) == [(11, "b", 1.0), (13, "d", 3.0)]
    users = C.map_frame(fit, "user", [5, 6, 7, 8], None, {"assign": torch.tensor([1, 0, -1, 1])})
    assert users.columns.tolist() == ["user_id", "x", "y", "cluster"] and users["cluster"].tolist() == [1, 0, -1, 1]


# ---- the planted cases ------------------------------------------------------------------------------------------------
KL_MARGIN = 0.04    # twice the largest gap to the fp64 run measured with this restatement (0.0192, 0.0028, 0.0067)


@pytest.mark.parametrize("case", range(3))
def test_planted_clusters_come_out_pure(case):
    clusters, per, D, perp = R.PLANTED[case]
    X, label = R.planted(clusters, per, D, case)
    n = len(X)
    Xd = X.astype(np.float64)
    d2 = 2.0 - 2.0 * Xd @ Xd.T                      # the input margins first, in fp64: every row's own cluster is nearer
    same = label[:, None] == label[None, :]
    np.fill_diagonal(d2, np.nan)
    assert np.nanmax(np.where(same, d2, np.nan)) < 0.75 * np.nanmin(np.where(~same, d2, np.nan))
    assert R.knn_purity(Xd, label) == 1.0 and per > 5
    off, idx, val = R.dense_affinities(X, perp)
    lr = R.auto_lr(n)
    assert lr == 50.0
    Y, V, G, info = R.fit(R.y0(n), off, idx, val, 500, lr=lr)
    assert info == 0 and np.isfinite(Y).all()
    assert R.knn_purity(Y, label) == 1.0
    P = R.dense_P(off, idx, val, n)
    Yf = R.fit_fp64(R.y0(n), P, 500, lr=lr)
    kl, klf = R.kl_fp64(Y, P), R.kl_fp64(Yf, P)
    print("case %d: fixed-point KL %.4f, plain fp64 KL %.4f" % (case, kl, klf))
    assert R.knn_purity(Yf, label) == 1.0 and abs(kl - klf) <= KL_MARGIN
