"""GPU tests of the split fold-in (anirec_fold_in_split, ops.fold_in_split).

Yardstick: the float64 NumPy restatement (tests/foldin_restatement.py) on the inputs of tests/foldin_split_cases.py — a
211-row table, one fitted row per list length 0, 1, 1023, 1024, 1025, 2048, 2049, 3079, 5000 (the chunk edges, one past
each, a ragged last chunk of 7, five chunks), step counts 0, 1, 2, 8, 50 (foldin_split_cases says why not 100).
Tolerance: foldin_cases.tolerances — 8 x the recorded distance of the FLOAT32 restatement from the float64 one, the
margin of tests/test_foldin_gpu.py; tests/test_foldin_split_cpu.py holds the float32 restatement inside that distance
on these very inputs.  The 100-step path is held exactly: a list of at most 1024 ratings gives the bits of
anirec_fold_in.
"""
import ctypes

import numpy as np
import pytest

import foldin_cases as K
import foldin_split_cases as S
import poison

pytestmark = pytest.mark.gpu
DEFAULT = ("binary_crossentropy", "sigmoid")
NAN_BITS = 0x7FC00000


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _head(act, dim=128):
    return dict(K.head_for(act, dim), activation=act)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _fold(fn, T, dim, loss, act, steps, off, idx, t, init):
    rows, ls = fn(_cuda(T), _head(act, dim), off, idx, t, init, lr=S.LR, steps=steps, l2=S.L2, loss=loss)
    return rows.cpu().numpy(), ls.cpu().numpy()


def _split(dim, loss, act, steps, off=None, idx=None, t=None, init=None):
    """ops.fold_in_split on a case's table and head -> (rows, loss) as NumPy arrays"""
    from anime_recommendations_amd import ops
    T, _, off0, idx0, t0, init0 = S.case_inputs(dim, loss, act)
    off, idx, t, init = (off0 if off is None else off, idx0 if idx is None else idx, t0 if t is None else t,
                         init0 if init is None else init)
    return _fold(ops.fold_in_split, T, dim, loss, act, steps, off, idx, t, init)


def _raw(dim, off, idx, t, init, steps, bufs=None, preset=None, chunk_map=None, ws_short=0, n_new=None):
    """anirec_fold_in_split itself on the default case's table: no wrapper check between the test and the kernel.
    ``bufs``: (rows, loss, err, workspace) tensors to write into (fresh ones otherwise); ``preset``: a 32-bit word the
    flag word holds on entry; ``chunk_map``: (chunk_offsets, chunk_row, n_chunks) instead of the builder's.
    Returns (status, rows, loss, err, workspace)."""
    import torch
    from anime_recommendations_amd import _lib, ops
    lib = _lib.load()
    T = _cuda(S.table(dim))
    n_new = len(off) - 1 if n_new is None else n_new
    c_off, c_row = ops.fold_chunk_map(off)
    n_chunks = int(c_off[-1])
    if chunk_map is not None:
        c_off, c_row, n_chunks = chunk_map
    if bufs is None:
        nb = int(lib.anirec_fold_in_split_workspace_bytes(S.N_TABLE, max(n_new, 0), n_chunks, dim))
        bufs = (torch.empty(max(n_new, 0), dim, dtype=torch.float32, device="cuda"),
                torch.empty(max(n_new, 0), dtype=torch.float32, device="cuda"),
                torch.empty(1, dtype=torch.int32, device="cuda"),
                torch.empty(nb - ws_short, dtype=torch.uint8, device="cuda"))
    rows, ls, err, ws = bufs
    if preset is not None:
        err.fill_(preset)
    d_off, d_idx, d_t, d_init = _cuda(np.asarray(off, np.int64)), _cuda(np.asarray(idx, np.int32)), \
        _cuda(np.asarray(t, np.float32)), _cuda(np.asarray(init, np.float32))
    d_coff, d_crow = _cuda(np.asarray(c_off, np.int32)), _cuda(np.asarray(c_row, np.int32))
    alpha = _cuda(S.alphas(steps)) if steps > 0 else None
    h = ops._head_struct(K.HEAD)
    st = lib.anirec_fold_in_split(_lib.ptr(T), dim, S.N_TABLE, ctypes.byref(h), 0, 0, S.L2, _lib.ptr(d_off), _lib.ptr(d_idx),
                                  _lib.ptr(d_t), n_new, _lib.ptr(d_coff), _lib.ptr(d_crow), n_chunks, _lib.ptr(d_init),
                                  _lib.ptr(alpha), steps, _lib.ptr(rows), _lib.ptr(ls), _lib.ptr(err), _lib.ptr(ws),
                                  ws.numel(), None)
    torch.cuda.synchronize()
    return st, rows, ls, err, ws


# ---- 1. parity with the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("dim,loss,act", S.CASES)
def test_parity_with_the_float64_restatement(dim, loss, act):
    ref = S.reference(dim, loss, act)
    init = S.case_inputs(dim, loss, act)[5]
    has = np.array(S.LENGTHS) > 0
    row_tol, loss_tol = K.tolerances(dim, loss, act)
    for steps in S.STEPS:
        rows, ls = _split(dim, loss, act, steps)
        want_rows, want_ls = ref[steps]
        d_row = np.abs(rows.astype(np.float64) - want_rows).max()
        d_loss = np.abs(ls[has].astype(np.float64) - want_ls[has]).max()
        print("fold_in_split parity dim %d %s %s steps %d: row %.3g (tol %.3g) loss %.3g (tol %.3g)"
              % (dim, loss, act, steps, d_row, row_tol, d_loss, loss_tol))
        assert d_row <= row_tol and d_loss <= loss_tol
        assert np.array_equal(_bits(rows[~has]), _bits(init[~has])) and np.isnan(ls[~has]).all()   # n == 0
        if steps == 0:
            assert np.array_equal(_bits(rows), _bits(init))


# ---- 2. a single chunk is anirec_fold_in --------------------------------------------------------------------
@pytest.mark.parametrize("dim", K.WIDTHS)
def test_single_chunk_lists_give_the_bits_of_fold_in(dim):
    """foldin_cases' users (lists of 0 .. 700 ratings) and the 1023- and 1024-rating lists of the new cases: rows and
    losses of ops.fold_in_split equal those of ops.fold_in bit for bit, at 100 steps too"""
    from anime_recommendations_amd import ops
    T, _, off, idx, t, init = K.case_inputs(dim, *DEFAULT)
    T2, _, off2, idx2, t2, init2 = S.case_inputs(dim, *DEFAULT)
    j0, j1 = S.LENGTHS.index(1023), S.LENGTHS.index(1024) + 1
    edge = (off2[j0:j1 + 1] - off2[j0], idx2[off2[j0]:off2[j1]], t2[off2[j0]:off2[j1]], init2[j0:j1])
    for steps in (0, 1, 8, 100):
        for table, args in ((T, (off, idx, t, init)), (T2, edge)):
            want = _fold(ops.fold_in, table, dim, *DEFAULT, steps, *args)
            got = _fold(ops.fold_in_split, table, dim, *DEFAULT, steps, *args)
            assert np.array_equal(_bits(got[0]), _bits(want[0])), steps
            assert np.array_equal(_bits(got[1]), _bits(want[1])), steps


def test_single_chunk_identity_under_another_head():
    """the same under mean_squared_error + tanh (another branch of the head switch), width 128"""
    from anime_recommendations_amd import ops
    case = (128, "mean_squared_error", "tanh")
    T, _, off, idx, t, init = K.case_inputs(*case)
    want = _fold(ops.fold_in, T, *case, 8, off, idx, t, init)
    got = _fold(ops.fold_in_split, T, *case, 8, off, idx, t, init)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))


# ---- 3. independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (32, 128))
def test_a_row_does_not_depend_on_the_call(dim):
    """every row of the case alone, in a batch of 60 in shuffled order (lengths up to 2500), and twice on the same
    buffers: the same bits"""
    _, _, off, idx, t, init = S.case_inputs(dim, *DEFAULT)
    steps = 8
    n_r = len(S.LENGTHS)
    base_rows, base_ls = _split(dim, *DEFAULT, steps)
    for j in range(n_r):                                                    # alone
        sl = slice(off[j], off[j + 1])
        rows, ls = _split(dim, *DEFAULT, steps, off=np.array([0, off[j + 1] - off[j]]), idx=idx[sl], t=t[sl], init=init[j:j + 1])
        assert np.array_equal(_bits(rows[0]), _bits(base_rows[j])) and np.array_equal(_bits(ls), _bits(base_ls[j:j + 1])), j
    rng = np.random.default_rng(7)                                          # among 51 others, shuffled
    lens = rng.integers(0, 2501, 60 - n_r)
    lists = [(idx[off[j]:off[j + 1]], t[off[j]:off[j + 1]], init[j]) for j in range(n_r)]
    for n in lens:
        lists.append((rng.integers(0, S.N_TABLE, n).astype(np.int32), (rng.integers(0, 11, n) / 10).astype(np.float32),
                      (rng.standard_normal(dim) * 0.05).astype(np.float32)))
    order = rng.permutation(60)
    b_off = np.concatenate([[0], np.cumsum([len(lists[o][0]) for o in order])]).astype(np.int64)
    rows, ls = _split(dim, *DEFAULT, steps, off=b_off, idx=np.concatenate([lists[o][0] for o in order]),
                      t=np.concatenate([lists[o][1] for o in order]), init=np.stack([lists[o][2] for o in order]))
    where = np.argsort(order)[:n_r]                                         # position of row j in the batch
    assert np.array_equal(_bits(rows[where]), _bits(base_rows)) and np.array_equal(_bits(ls[where]), _bits(base_ls))
    st, r1, l1, e1, ws = _raw(dim, off, idx, t, init, steps)                # twice on the same buffers
    assert st == 0
    first = (r1.clone(), l1.clone())
    st, r2, l2, e2, _ = _raw(dim, off, idx, t, init, steps, bufs=(r1, l1, e1, ws))
    assert st == 0 and int(e2.item()) == 0
    assert np.array_equal(_bits(first[0].cpu().numpy()), _bits(r2.cpu().numpy()))
    assert np.array_equal(_bits(first[1].cpu().numpy()), _bits(l2.cpu().numpy()))
    assert np.array_equal(_bits(r2.cpu().numpy()), _bits(base_rows))        # and the raw call is the wrapper's


# ---- 4. errors, through the raw entry point --------------------------------------------------------------------
def _clean(dim, steps=8):
    _, _, off, idx, t, init = S.case_inputs(dim, *DEFAULT)
    st, rows, ls, err, _ = _raw(dim, off, idx, t, init, steps, preset=0x7F7F7F7F)
    assert st == 0 and int(err.item()) == 0                                 # the flag word is overwritten, not or-ed
    return (off, idx, t, init), rows.cpu().numpy(), ls.cpu().numpy()


@pytest.mark.parametrize("dim", (32, 128))
def test_bad_index_and_decreasing_offsets_poison_one_row_only(dim):
    (off, idx, t, init), rows0, ls0 = _clean(dim)
    n_r = len(S.LENGTHS)
    for what in ("index past the table", "negative index", "decreasing offsets"):
        o, i = off.copy(), idx.copy()
        skip = []
        if what == "index past the table":
            victim = 8
            i[off[8] + 4999] = S.N_TABLE                                    # in the last chunk of the 5000-rating list
        elif what == "negative index":
            victim = 6
            i[off[6] + 1500] = -1                                           # in the second chunk of the 2049
        else:
            victim = 4                                                      # offsets[5] < offsets[4]: row 4's pair decreases;
            o[5] = off[4] - 3                                               # row 5 now spans row 4's ratings and its own
            skip = [5]
        for preset in (0, 0x7F7F7F7F):
            st, rows, ls, err, _ = _raw(dim, o, i, t, init, 8, preset=preset)
            assert st == 0 and int(err.item()) == 1, what
            rows, ls = rows.cpu().numpy(), ls.cpu().numpy()
            assert (_bits(rows[victim]) == NAN_BITS).all() and _bits(ls[victim:victim + 1])[0] == NAN_BITS, what
            same = [j for j in range(n_r) if j != victim and j not in skip]
            assert np.array_equal(_bits(rows[same]), _bits(rows0[same])) and np.array_equal(_bits(ls[same]), _bits(ls0[same])), what


@pytest.mark.parametrize("dim", (32, 128))
def test_a_wrong_chunk_map_poisons_every_row(dim):
    from anime_recommendations_amd import ops
    (off, idx, t, init), rows0, ls0 = _clean(dim)
    c_off, c_row = ops.fold_chunk_map(off)
    n_chunks = int(c_off[-1])
    maps = {}
    m = c_off.copy()
    m[5] += 1                                                               # one pair off by one: rows 4 and 5 miscounted
    maps["pair off by one"] = (m, c_row, n_chunks)
    for name, bad in (("chunk_row past the rows", len(off) - 1), ("negative chunk_row", -1), ("chunk_row of a neighbour", 7)):
        r = c_row.copy()
        r[-1] = bad                                                         # the last chunk of the 5000-rating list
        maps[name] = (c_off, r, n_chunks)
    maps["too few chunks"] = (c_off, c_row[:-1], n_chunks - 1)
    m = c_off + 1                                                           # the right counts from a wrong start
    maps["prefix sums from 1"] = (m, np.concatenate([[0], c_row]).astype(np.int32), n_chunks + 1)
    for name, cmap in maps.items():
        for preset in (0, 0x7F7F7F7F):
            st, rows, ls, err, _ = _raw(dim, off, idx, t, init, 8, preset=preset, chunk_map=cmap)
            assert st == 0 and int(err.item()) == 1, name
            assert (_bits(rows.cpu().numpy()) == NAN_BITS).all() and (_bits(ls.cpu().numpy()) == NAN_BITS).all(), name


def test_bad_arguments_are_refused_and_write_nothing():
    import torch
    from anime_recommendations_amd import _lib, ops
    dim = 64
    _, _, off, idx, t, init = S.case_inputs(dim, *DEFAULT)
    n_new = len(off) - 1
    c_off, c_row = ops.fold_chunk_map(off)
    nb = int(_lib.load().anirec_fold_in_split_workspace_bytes(S.N_TABLE, n_new, int(c_off[-1]), dim))

    def bufs(short=0):
        return (torch.full((n_new, dim), 7.0, device="cuda"), torch.full((n_new,), 7.0, device="cuda"),
                torch.full((1,), 7, dtype=torch.int32, device="cuda"), torch.zeros(nb - short, dtype=torch.uint8, device="cuda"))

    def untouched(st, rows, ls, err):
        return st == -1 and bool((rows == 7).all()) and bool((ls == 7).all()) and int(err.item()) == 7

    st, rows, ls, err, _ = _raw(dim, off, idx, t, init, 8, bufs=bufs(short=1))          # a workspace one byte short
    assert untouched(st, rows, ls, err)
    st, rows, ls, err, _ = _raw(dim, off, idx, t, init, 8, bufs=bufs(), chunk_map=(c_off, c_row, -1))
    assert untouched(st, rows, ls, err)
    st, rows, ls, err, _ = _raw(48, off, idx, t, init, 8, bufs=bufs())                  # no such width
    assert untouched(st, rows, ls, err)
    st, rows, ls, err, _ = _raw(dim, off, idx, t, init, -1, bufs=bufs())
    assert untouched(st, rows, ls, err)
    st, rows, ls, err, _ = _raw(dim, off, idx, t, init, 8, bufs=bufs(), n_new=-1)
    assert untouched(st, rows, ls, err)
    st, rows, ls, err, _ = _raw(dim, off, idx, t, init, 8, bufs=bufs(), n_new=0)        # no rows: OK, nothing enqueued
    assert st == 0 and bool((rows == 7).all()) and bool((ls == 7).all()) and int(err.item()) == 7


def test_wrapper_refuses_what_fold_in_refuses():
    from anime_recommendations_amd import ops
    T, head, off, idx, t, init = S.case_inputs(32, *DEFAULT)
    tT = _cuda(T)
    with pytest.raises(ValueError, match="loss"):
        ops.fold_in_split(tT, _head("sigmoid"), off, idx, t, init, loss="hinge")
    with pytest.raises(ValueError, match="activation"):
        ops.fold_in_split(tT, dict(K.HEAD, activation="gelu"), off, idx, t, init)
    with pytest.raises(ValueError, match="steps"):
        ops.fold_in_split(tT, _head("sigmoid"), off, idx, t, init, steps=-1)
    with pytest.raises(ValueError, match="offsets"):
        ops.fold_in_split(tT, _head("sigmoid"), off[::-1].copy(), idx, t, init)
    bad = idx.copy()
    bad[-1] = S.N_TABLE
    with pytest.raises(ValueError, match="out of range"):
        ops.fold_in_split(tT, _head("sigmoid"), off, bad, t, init, steps=2)
    rows, ls = ops.fold_in_split(tT, _head("sigmoid"), [0], [], [], np.zeros((0, 32), np.float32))       # no rows
    assert rows.shape == (0, 32) and ls.shape == (0,)
    rows, ls = ops.fold_in_split(tT, _head("sigmoid"), [0, 0, 0], [], [], init[:2], steps=3)             # no chunks
    assert np.array_equal(_bits(rows.cpu().numpy()), _bits(init[:2])) and np.isnan(ls.cpu().numpy()).all()


# ---- 5. dirty memory -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", poison.ORDER)
def test_dirty_workspace_and_outputs(byte):
    """the workspace, the outputs and the flag word hold ``byte`` in every byte on entry: the same results"""
    import torch
    from anime_recommendations_amd import _lib, ops
    for dim in (32, 256):
        (off, idx, t, init), rows0, ls0 = _clean(dim)
        log = []
        with poison.poisoned(byte, log):
            rows, ls = _split(dim, *DEFAULT, 8)
        assert len(log) >= 4 and sum(log) >= S.N_TABLE * dim * 4            # rows, loss, flag word, workspace
        assert np.array_equal(_bits(rows), _bits(rows0)) and np.array_equal(_bits(ls), _bits(ls0))
        n_new = len(off) - 1
        n_chunks = int(ops.fold_chunk_map(off)[0][-1])
        nb = int(_lib.load().anirec_fold_in_split_workspace_bytes(S.N_TABLE, n_new, n_chunks, dim))
        bufs = (poison.fill(torch.empty(n_new, dim, dtype=torch.float32, device="cuda"), byte),
                poison.fill(torch.empty(n_new, dtype=torch.float32, device="cuda"), byte),
                poison.fill(torch.empty(1, dtype=torch.int32, device="cuda"), byte),
                poison.fill(torch.empty(nb, dtype=torch.uint8, device="cuda"), byte))
        st, rows, ls, err, _ = _raw(dim, off, idx, t, init, 8, bufs=bufs)
        assert st == 0 and int(err.item()) == 0
        assert np.array_equal(_bits(rows.cpu().numpy()), _bits(rows0)) and np.array_equal(_bits(ls.cpu().numpy()), _bits(ls0))
