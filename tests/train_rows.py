"""A row-relative bar for the train step's moments (a helper module, no tests of its own).

After an Adam step W moves by about +-lr whatever the gradient's size, so the moments M and V are the only place where
a wrong per-row gradient sum shows; and a table-wide `atol = 1e-4 * max|want|` is set by the heaviest row: a row whose
largest |M| is 5e-3 of the table's has a bar of 2 % of itself, and a row whose largest V is 2e-5 of the table's has no
bar at all.  Here every row is held to a multiple of its OWN largest element:

    max|got[r] - o64[r]|  <=  K * unit * max|o64[r]|

o64 is oracle.anirec_oracle.train_step in fp64, `unit` the largest such ratio of the fp32 oracle over the rows of the
table (`row_unit`: measured on the two references, never on the kernel) and K a small multiple for a summation order
that is not NumPy's.

`run_length_batch` is the batch the bar is made for: runs of 1 ... 65 ratings per row in both tables, which is every
ragged remainder of a 32-contribution chunk at every lane dealing of k_bwd (8, 16, 32 or 64 lanes per row holding
4, 2, 1 or 1 contributions each: the remainder edges are 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32 at D = 32 and
16 +- 1 at D = 64) and rows of one, two and three chunks.

Measured on the CPU for run_length_batch(D, 0), Adam, one step: `unit`, the largest row ratio of the fp32 oracle to the
fp64 one (at 64 the one-rating user row sets mU and vU), and in brackets the furthest the fp32 oracle goes, in units,
over 20 other orders of the same batch:

    D     mU               mA               vU               vA
    32    5.06e-7 (1.10)   5.42e-7 (1.20)   7.52e-7 (1.53)   9.82e-7 (1.16)
    64    2.09e-6 (1.24)   4.66e-7 (1.21)   4.18e-6 (1.23)   7.35e-7 (1.43)
    128   3.29e-7 (1.68)   6.93e-7 (0.74)   6.07e-7 (1.72)   1.24e-6 (0.72)
    256   3.56e-7 (1.36)   4.16e-7 (1.27)   6.40e-7 (1.36)   7.20e-7 (1.25)

Measured on an MI355X, the same batch: kernel / fp32 oracle, each the largest row ratio to the fp64 oracle (the figure
check_rows returns, in units):

    D     Adam mU  mA    vU    vA      RMSprop vU  vA      Adagrad vU  vA
    32         0.60  0.63  0.74  0.60          0.82  0.61          1.00  1.00
    64         1.74  0.78  1.73  0.71          1.73  0.73          1.00  1.00
    128        1.12  0.53  1.05  0.56          1.04  0.53          1.00  1.00
    256        1.28  0.88  1.22  1.03          1.29  1.01          1.00  1.00

(Adagrad's V is 0.1 + g^2 with g^2 below 1e-6: the unit, 5.2e-8, is the rounding of 0.1.)  Every ratio is below 2, so K
keeps the project's 4 (test_train_edges_gpu.K64); K * unit is 1.7e-5 at most, 1 / 230 of LOST_ONE.
"""
import functools

import numpy as np

from oracle import anirec_oracle as orc

f32 = np.float32
LR = 3e-5
N_U, N_A, RUNS = 80, 70, 65
N = RUNS * (RUNS + 1) // 2                  # 2145 ratings
HEAD_W = 1.2
MOMENTS = ("mU", "mA", "vU", "vA")
# the multiple of `unit`: test_train_edges_gpu.K64, the allowance for a chunked summation order (32 ratings, then the
# chunks in order) against NumPy's pairwise one
K = 4.0
# no bar may reach a quarter of one contribution of 65 equal ones: above that, one lost contribution of the longest run
# could pass
LOST_ONE = 1.0 / (4 * RUNS)


def run_length_batch(D, seed=0):
    """(U, A, ui, ai, t): user row r has r + 1 ratings (r = 0 ... 64), the anime indices are a permutation of the same
    multiset, so every run length 1 ... 65 occurs in both tables; rows 65 ... of each table stay untouched"""
    rng = np.random.default_rng([seed, D])
    ui = np.repeat(np.arange(RUNS), np.arange(1, RUNS + 1)).astype(np.int64)
    ai = rng.permutation(ui)
    U = rng.uniform(-0.05, 0.05, (N_U, D)).astype(f32)
    A = rng.uniform(-0.05, 0.05, (N_A, D)).astype(f32)
    t = (rng.integers(0, 11, N) / 10).astype(f32)
    for idx in (ui, ai):
        rows, cnt = np.unique(idx, return_counts=True)
        assert len(idx) == N and rows.max() == RUNS - 1 and sorted(cnt.tolist()) == list(range(1, RUNS + 1))
    return U, A, ui, ai, t


def oracle_step(U, A, ui, ai, t, dtype=f32, optimizer="adam", head=None, lr=LR):
    """the state after ONE orc.train_step from initialisation, in `dtype` (test_train_edges_gpu._oracle's way of
    running the oracle in fp64), and the step's metrics"""
    st = orc.new_state(U.astype(dtype), A.astype(dtype), orc.new_head(**(head or dict(w=HEAD_W))), optimizer=optimizer)
    if dtype is not f32:
        for k in ("mU", "vU", "mA", "vA"):
            st[k] = st[k].astype(dtype)
        st["head"] = {k: np.asarray(v, dtype) if np.ndim(v) else dtype(v) for k, v in st["head"].items()}
    met = orc.train_step(st, ui, ai, t, lr, dtype=dtype)[0]
    return st, met


class RowMiss(AssertionError):
    """a row outside its bar: .table, .row, .run (the row's run length, None without the batch's indices)"""

    def __init__(self, msg, table, row, run):
        super().__init__(msg)
        self.table, self.row, self.run = table, row, run


def _row_ratio(x, o64):
    """per row max|x[r] - o64[r]| / max|o64[r]| (0 where the fp64 row is all zero), in fp64"""
    o64 = np.asarray(o64, np.float64)
    d = np.abs(np.asarray(x, np.float64) - o64).max(1)
    m = np.abs(o64).max(1)
    return np.divide(d, m, out=np.zeros_like(d), where=m > 0), d, m


def row_unit(o32, o64, keys=MOMENTS, keep=None):
    """{moment: the largest row ratio of the fp32 oracle's state against the fp64 one}; keep: {moment: mask of the
    rows that count} where some are held by another bar"""
    keep = keep or {}
    return {k: float(_row_ratio(o32[k], o64[k])[0][keep.get(k, slice(None))].max()) for k in keys}


def run_lengths(idx, n_rows):
    return np.bincount(np.asarray(idx, np.int64), minlength=n_rows)


def check_rows(got, o64, unit, K, what, idx=None, keep=None, figures=None):
    """every row of `got` within K * unit of its own largest fp64 element; rows whose fp64 row is all zero exactly
    zero.  A miss names the table, the WORST row (largest distance in units of its bar) and, given the batch's indices
    into this table, its run length.  keep: a mask of the rows to hold (all).  Returns the largest row ratio in units
    of `unit`, and leaves it in figures[what] before it asserts anything."""
    got = np.asarray(got)
    assert got.shape == np.shape(o64), (what, got.shape, np.shape(o64))
    ratio, d, m = _row_ratio(got, o64)
    if keep is not None:
        ratio, d, m = (np.where(keep, x, 0.0) for x in (ratio, d, m))
        got = np.where(np.asarray(keep)[:, None], got, 0)
    if figures is not None:
        figures[what] = float(ratio.max() / unit) if unit > 0 else 0.0
    assert np.isfinite(got).all(), what
    runs = run_lengths(idx, len(got)) if idx is not None else None
    zero = m == 0
    if zero.any() and np.abs(np.asarray(got)[zero]).max() != 0:
        r = int(np.nonzero(zero & (np.abs(got).max(1) != 0))[0][0])
        raise RowMiss("%s: row %d is zero in the fp64 oracle, got max |x| %.3e" % (what, r, np.abs(got[r]).max()),
                      what, r, None if runs is None else int(runs[r]))
    bar = K * unit
    bad = np.nonzero(ratio > bar)[0]
    if len(bad):
        r = int(bad[np.argmax(ratio[bad])])
        raise RowMiss(
            "%s: row %d%s is %.3e of its largest element (%.3e) from the fp64 oracle, the bar is %.1f x %.3e = %.3e; "
            "%d rows miss it: %s" % (what, r, "" if runs is None else " (run length %d)" % runs[r], ratio[r], m[r], K,
                                     unit, bar, len(bad), bad[:16].tolist()),
            what, r, None if runs is None else int(runs[r]))
    return float(ratio.max() / unit) if unit > 0 else 0.0


def check_table_wide(got, o64, rows=None):
    """the bar this module tightens, `atol = 1e-4 * max|want|` over the whole table: True where `rows` (all) pass"""
    o64 = np.asarray(o64, np.float64)
    d = np.abs(np.asarray(got, np.float64) - o64)
    if rows is not None:
        d = d[np.asarray(rows)]
    return bool(d.max() <= 1e-4 * np.abs(o64).max())


@functools.lru_cache(maxsize=None)
def reference(D, optimizer="adam", seed=0):
    """(batch, fp32 state, fp64 state, fp32 metrics, unit) of run_length_batch(D, seed): computed once, shared, and
    left unchanged by every user"""
    batch = run_length_batch(D, seed)
    o32, met = oracle_step(*batch, dtype=f32, optimizer=optimizer)
    o64, _ = oracle_step(*batch, dtype=np.float64, optimizer=optimizer)
    keys = MOMENTS if optimizer == "adam" else () if optimizer == "sgd" else ("vU", "vA")
    return batch, o32, o64, met, row_unit(o32, o64, keys)
