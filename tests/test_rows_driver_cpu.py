"""CPU tests of the score-row driver (recs.rows_topk_batched / rows_rank_batched) and of the six wrappers'
refusals, with ``ops`` replaced by the restatements (``fuse_host_ops``): 11 lists x 70 items, so three watched words with a
ragged last one, and targets on 4 of the lists, the first and the last among them."""
import numpy as np
import pytest
import torch

import cooc_restatement as CR
from test_fuse_cpu import fuse_host_ops, host_ops  # noqa: F401  (ops as the restatements on CPU tensors)

from anime_recommendations_amd import ops, recs

NL, N, K = 11, 70, 5
BATCHES = (1, 3, 4, 11, 16)


def _case():
    rng = np.random.default_rng(17)
    rows = rng.choice(np.float32([-1.5, 0.0, 0.25, 2.0, 7.0]), (NL, N))          # ties in every row
    vec = rng.integers(0, 6, N).astype(np.float32)
    W = rng.random((NL, N)) < 0.3
    tr = np.array([10, 0, 3, 7, 0, 10, 3])
    ta = rng.integers(0, N, len(tr))
    return rows, vec, W, CR.pack_bits(W).view(np.int32), tr, ta


def _counted(rows):
    calls = []

    def source(l0, l1):
        calls.append((l0, l1))
        return torch.as_tensor(rows[l0:l1])
    return source, calls


def _bits(x):
    return x.numpy().view(np.uint32)


@pytest.mark.parametrize("kind", ("callable", "vector"))
def test_every_batch_equals_the_single_span(fuse_host_ops, kind):  # noqa: F811
    rows, vec, W, wb, tr, ta = _case()
    keep = (np.arange(N) % 5 != 2).astype(np.uint8)
    whole = torch.as_tensor(rows if kind == "callable" else np.broadcast_to(vec, (NL, N)).copy())
    want_i, want_s = ops.rows_topk(whole, K, keep=keep, wbits=wb)
    want_r = ops.rows_rank(whole, tr, ta, wb)
    for batch in BATCHES:
        source, calls = _counted(rows) if kind == "callable" else (torch.as_tensor(vec), None)
        idx, sc = recs.rows_topk_batched(source, NL, K, wb, keep, batch=batch)
        assert idx.dtype == torch.int32 and sc.dtype == torch.float32 and idx.shape == sc.shape == (NL, K)
        assert torch.equal(idx, want_i) and np.array_equal(_bits(sc), _bits(want_s)), batch
        if calls is not None:
            assert calls == [(l0, min(NL, l0 + batch)) for l0 in range(0, NL, batch)]
            del calls[:]
        rank = recs.rows_rank_batched(source, NL, wb, tr, ta, batch=batch)
        assert rank.dtype == torch.int32 and torch.equal(rank, want_r), batch
        if calls is not None:       # a span without targets is not scored
            assert calls == [(l0, min(NL, l0 + batch)) for l0 in range(0, NL, batch) if ((tr >= l0) & (tr < l0 + batch)).any()]
    # no mask at all
    source = _counted(rows)[0] if kind == "callable" else torch.as_tensor(vec)
    idx, sc = recs.rows_topk_batched(source, NL, K, batch=4)
    want = ops.rows_topk(whole, K)
    assert torch.equal(idx, want[0]) and np.array_equal(_bits(sc), _bits(want[1]))
    assert torch.equal(recs.rows_rank_batched(source, NL, None, tr, ta, batch=4), ops.rows_rank(whole, tr, ta))


def test_only_spans_that_hold_a_target_are_scored(fuse_host_ops):  # noqa: F811
    rows, _, _, wb, tr, ta = _case()
    source, calls = _counted(rows)
    recs.rows_rank_batched(source, NL, wb, tr, ta, batch=1)
    assert len(set(tr.tolist())) == 4 and calls == [(0, 1), (3, 4), (7, 8), (10, 11)]      # 4 calls, not 11
    del fuse_host_ops[:]
    assert recs.rows_rank_batched(source, NL, wb, [], [], batch=1).numel() == 0
    assert len(calls) == 4 and fuse_host_ops == []                      # no target: no row, no GPU call


def test_empty_results_keep_their_dtypes(fuse_host_ops):  # noqa: F811
    rows, vec, _, wb, tr, ta = _case()
    for source in (_counted(rows)[0], torch.as_tensor(vec)):
        for device in (None, "cpu"):
            idx, sc = recs.rows_topk_batched(source, 0, K, wb[:0], device=device)
            assert idx.shape == sc.shape == (0, K) and idx.dtype == torch.int32 and sc.dtype == torch.float32
            rank = recs.rows_rank_batched(source, NL, wb, [], [], device=device)
            assert rank.shape == (0,) and rank.dtype == torch.int32
            rank = recs.rows_rank_batched(source, 0, wb[:0], [], [], device=device)
            assert rank.shape == (0,) and rank.dtype == torch.int32
    knn = dict(nbr_idx=torch.zeros(N, 2, dtype=torch.int32), nbr_sim=torch.zeros(N, 2))
    fit = dict(X=torch.zeros(4, 8), Y=torch.zeros(N, 8))
    for idx, sc in (recs.itemknn_topk(knn, [0], [], None, K), recs.als_topk(fit, [], K),
                    recs.hybrid_topk([torch.as_tensor(vec)], K, n_lists=0)):
        assert idx.shape == sc.shape == (0, K) and idx.dtype == torch.int32 and sc.dtype == torch.float32
    for rank in (recs.itemknn_rank(knn, [0, 0], [], None, None, [], []), recs.als_rank(fit, [1], None, [], []),
                 recs.hybrid_rank([torch.as_tensor(vec)], wb, [], [])):
        assert rank.shape == (0,) and rank.dtype == torch.int32


def test_refusals_carry_the_callers_name_and_the_wrappers_keep_their_texts(fuse_host_ops):  # noqa: F811
    rows, vec, W, wb, tr, ta = _case()
    source = _counted(rows)[0]
    for batch in (0, -3):
        with pytest.raises(ValueError, match="^my_lists: batch must be >= 1"):
            recs.rows_topk_batched(source, NL, K, wb, batch=batch, what="my_lists")
        with pytest.raises(ValueError, match="^my_ranks: batch must be >= 1"):
            recs.rows_rank_batched(source, NL, wb, tr, ta, batch=batch, what="my_ranks")
    with pytest.raises(ValueError, match="^my_ranks: target_row out of range"):
        recs.rows_rank_batched(source, NL, wb, [NL], [0], what="my_ranks")
    with pytest.raises(ValueError, match="^my_ranks: target_row out of range"):
        recs.rows_rank_batched(source, NL, wb, [-1], [0], what="my_ranks")
    with pytest.raises(ValueError, match="^my_ranks: target_row and target_anime must have one entry per target"):
        recs.rows_rank_batched(source, NL, wb, [0, 1], [0], what="my_ranks")
    assert fuse_host_ops == []                                          # every refusal before a row is scored
    knn = dict(nbr_idx=torch.zeros(N, 2, dtype=torch.int32), nbr_sim=torch.zeros(N, 2))
    off, hist = np.arange(NL + 1), np.arange(NL)
    fit = dict(X=torch.zeros(NL, 8), Y=torch.zeros(N, 8))
    users = np.arange(NL)
    st, sa = np.nonzero(W)
    cases = ((lambda: recs.itemknn_topk(knn, [], hist), "itemknn: offsets holds n_lists \\+ 1 entries"),
             (lambda: recs.itemknn_rank(knn, [], hist, None, wb, tr, ta), "itemknn: offsets holds n_lists \\+ 1 entries"),
             (lambda: recs.itemknn_rows_source(knn, [], hist), "itemknn: offsets holds n_lists \\+ 1 entries"),
             (lambda: recs.itemknn_topk(knn, off, hist, None, K, wb, batch=0), "itemknn_topk: batch must be >= 1"),
             (lambda: recs.itemknn_rank(knn, off, hist, None, wb, [NL], [0]), "itemknn_rank: target_row out of range"),
             (lambda: recs.itemknn_rank(knn, off, hist, None, wb, [0], [0, 1]), "itemknn_rank: target_row and target_anime"),
             (lambda: recs.als_topk(fit, [0, NL], K), "als: user out of range"),
             (lambda: recs.als_rank(fit, [-1], wb, tr, ta), "als: user out of range"),
             (lambda: recs.als_rows_source(fit, [NL]), "als: user out of range"),
             (lambda: recs.als_topk(fit, users, K, wb, batch=0), "als_topk: batch must be >= 1"),
             (lambda: recs.als_rank(fit, users, wb, tr, ta, batch=0), "als_rank: batch must be >= 1"),
             (lambda: recs.als_rank(fit, users, wb, [NL], [0]), "als_rank: target_row out of range"),
             (lambda: recs.als_rank(fit, users, wb, [0], []), "als_rank: target_row and target_anime must have one entry"),
             (lambda: recs.hybrid_topk([source], K), "hybrid_topk: n_lists is needed without watched_bits"),
             (lambda: recs.hybrid_topk([source], K, watched_bits=wb, batch=0), "hybrid_topk: batch must be >= 1"),
             (lambda: recs.hybrid_rank([source], None, tr, ta), "hybrid_rank: watched_bits .* is needed"),
             (lambda: recs.hybrid_rank([source], wb, tr, ta, batch=0), "hybrid_rank: batch must be >= 1"),
             (lambda: recs.hybrid_rank([source], wb, [NL], [0]), "hybrid_rank: target_row out of range"),
             (lambda: recs.hybrid_rank([source], wb, [0], [96]), "hybrid_rank: target_anime out of range"),
             (lambda: recs.hybrid_rank([source], wb, [0, 1], [0]), "hybrid_rank: target_row and target_anime must have one"),
             (lambda: recs.hybrid_rank([source], wb, [int(st[0])], [int(sa[0])]),
              "hybrid_rank: a target has its own watched bit set \\(a fused row holds no value there\\)"))
    for call, text in cases:
        with pytest.raises(ValueError, match="^" + text):
            call()
    assert fuse_host_ops == []
    # the other two rank a target under its own watched bit: only the hybrid refuses it
    assert recs.als_rank(fit, users, wb, [int(st[0])], [int(sa[0])]).numel() == 1
