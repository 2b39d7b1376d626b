"""The launch-cap cases (DESIGN.md "Launch caps") held to the caps in the sources, without a device.

tests/test_launch_caps_gpu.py runs every capped or split launch just past its cap.  Its shapes mirror constants of the
``.hip`` files; here each constant is read from the source text and each shape is shown to be past its cap, and not past
it with one pass fewer.  A change that moves a cap fails here, instead of silently turning the GPU cases back into
one-pass cases.  The inputs and restatements that need no device run here too, with the conditions the GPU tests rest
on: rows shared between passes, the bad query in the second launch, the lattice terms exactly zero.
"""
import numpy as np

import launch_caps_cases as L


def test_the_caps_are_the_ones_the_shapes_were_chosen_for():
    c = L.caps()
    assert (c["bpr_blocks"], c["bpr_lanes"], c["bpr_sample_blocks"]) == (4096, 1024, 65536)
    assert (c["km_grid"], c["km_threads"], c["km_image"], c["km_two_lanes_above"]) == (1024, 256, 32768, 128)
    assert (c["cooc_tiles"], c["cooc_tile"], c["wcooc_tiles"], c["wcooc_tile"]) == (32768, 64, 32768, 64)
    assert (c["tsne_init_blocks"], c["tsne_threads"]) == (1024, 256)
    assert (c["ing_minmax_blocks"], c["ing_init_blocks"], c["ing_id_max_blocks"], c["ing_id_max_rows"]) == (2048, 2048, 2048, 4096)
    assert c["ing_rows_blocks"] == 16384
    assert (c["boot_blocks"], c["rownorm_blocks"], c["rownorm_floats"]) == (65536, 4096, 1024)


def test_bpr_batches_are_past_the_cap_by_the_passes_stated():
    want = {256: 3, 32: 2, 128: 2}
    assert sorted(w for w, _ in L.BPR_CASES) == sorted(want)
    for width, batch in L.BPR_CASES:
        per = L.bpr_pass_slots(width)
        assert L.passes(batch, per) == want[width], (width, batch, per)
        assert batch % per < per // 2 and batch % per != 0      # the last pass is a partial one
        assert L.passes(batch - batch % per, per) == want[width] - 1
    assert L.bpr_pass_slots(64) == 65536                         # the width recs.bpr_fit's default batch strides at


def test_bpr_later_passes_share_rows_with_the_first():
    """the count exchange across passes, in both steps: more than one kept slot of a later pass touches a row that a
    first-pass slot touched.  The width-128 case has ONE slot past the first pass; there the slot is kept and all three
    of its rows are shared, so more than one count is exchanged across the passes all the same."""
    for width, batch in L.BPR_CASES:
        later = batch - L.bpr_pass_slots(width)
        for step in range(L.BPR_STEPS["n_steps"]):
            kept, slots, touches = L.bpr_shared_rows(width, batch, step)
            what = (width, batch, step, kept, slots, touches)
            if later > 1:
                assert slots > 1 and touches > 3, what
            else:
                assert (kept, slots, touches) == (1, 1, 3), what


def test_bpr_sparse_case_has_rows_that_only_the_later_pass_updates():
    p = L.BPR_SPARSE
    per = L.bpr_pass_slots(p["width"])
    assert L.passes(p["batch"], per) == 2 and p["batch"] - per == 300
    X, Y, counts, err, own = L.bpr_sparse_ref()
    X0, _ = L.bpr_sparse_tables()
    assert err == 0 and counts[0, 0] > p["batch"] * 0.9
    assert len(own) > 100 and (X[own] != X0[own]).any(axis=1).all()       # moved, and by a slot of the later pass alone


def test_bpr_restatement_of_the_cases():
    off, idx, pu = L.bpr_lists()
    lens = np.diff(off)
    assert len(lens) == L.BPR_USERS and lens.min() == 1 and lens.max() == 60 and idx.max() < L.BPR_ITEMS
    for width, batch in L.BPR_CASES:
        X, Y, counts, err = L.bpr_ref(width, batch)
        X0, Y0 = L.bpr_tables(width)
        assert err == 0 and counts.shape == (2, 3) and (counts[:, 0] + counts[:, 1] == batch).all()
        assert counts[:, 0].min() > batch // 2 and (X[:, -1] == 1.0).all()
        assert (X != X0).any(axis=1).sum() > 500 and (Y != Y0).any(axis=1).sum() > 800          # most rows moved


def test_sampler_steps_lie_where_the_case_says():
    p, per = L.SAMPLE, L.sample_pass_entries()
    total = p["n_steps"] * p["batch"]
    assert per == 16777216 and L.passes(total, per) == 2 and L.passes(total - p["batch"], per) == 1
    assert 16 * p["batch"] >= per                               # step 16: every slot past the first pass
    assert 15 * p["batch"] < per                                # steps 0 .. 15: inside it
    assert L.SAMPLE_CHECKED == (0, 15, 16) and total * 12 == 204 * 2 ** 20
    trip = L.sample_ref(16)
    assert trip.shape == (p["batch"], 3) and (trip[:, 0] >= 0).all() and (trip[:, 2] >= 0).mean() > 0.9
    assert not np.array_equal(trip, L.sample_ref(15))


def test_kmeans_rows_are_past_the_cap():
    a, b = L.KM_A, L.KM_B
    assert L.km_pass_rows(a["dim"]) == 262144 and L.km_pass_rows(b["dim"]) == 131072
    assert a["k"] <= L.km_tile(a["dim"]) and b["k"] == L.km_tile(b["dim"]) + 1      # one tile; two tiles
    for case in (a, b):
        per = L.km_pass_rows(case["dim"])
        rows_per_batch = per // L.caps()["km_grid"]
        assert L.passes(case["n_rows"], per) == 2 and L.passes(case["n_rows"] - case["n_rows"] % per, per) == 1
        assert case["n_rows"] % per > rows_per_batch             # two workgroups take a second batch, the last one partial
        assert case["n_rows"] % rows_per_batch != 0
        bad, ta, tb = L.km_planted(case)
        assert per <= bad < ta < tb < case["n_rows"] and ta // rows_per_batch != tb // rows_per_batch
    # k_kmeans_init and k_kmeans_count take one row a lane at every width: the fit case strides them too
    assert L.passes(a["n_rows"], L.caps()["km_grid"] * L.caps()["km_threads"]) == 2


def test_cooc_queries_make_a_second_launch_with_the_bad_query_in_it():
    c, p = L.caps(), L.COOC
    for tiles, tile in ((c["cooc_tiles"], c["cooc_tile"]), (c["wcooc_tiles"], c["wcooc_tile"])):
        per = tiles * tile
        assert per == 2097152 and L.passes(p["nq"], per) == 2 and L.passes(p["nq"] - 70, per) == 1
        assert L.passes(p["nq"] - per, tile) == 2 and (p["nq"] - per) % tile == 6    # two tiles, the last one partial
        assert L.COOC_BAD_AT >= per + tile                       # the bad query: second launch, last tile
    bits, queries, row, user_q, rs, cs = L.cooc_inputs()
    assert queries[L.COOC_BAD_AT] == p["bad_query"] >= p["n_items"] and row[L.COOC_BAD_AT] == p["n_items"]
    good = np.delete(queries, L.COOC_BAD_AT)
    assert good.min() == 0 and good.max() == p["n_items"] - 1 and np.array_equal(queries[:10] % 5, np.arange(10) % 5)
    assert np.array_equal(L.cooc_distinct()[row], queries)
    assert L.cooc_tile_rows(32769) == slice(2097216, p["nq"])


def test_cooc_and_wcooc_restatements_of_the_distinct_queries():
    n = L.COOC["n_items"]
    sim, cnt, excl, pop, err = L.cooc_ref()
    assert err == 1 and sim.shape == (6, n) and np.isnan(sim[5]).all() and (cnt[5] == -1).all() and excl[5, 0] == (1 << n) - 1
    assert np.isfinite(sim[:5]).all() and (sim[:5] > 0).any() and (sim[:5] == 0).any() and (cnt[:5] >= 0).all()
    assert all(excl[q, 0] >> q & 1 for q in range(n)) and excl[4, 0] == (1 << n) - 1 and pop[4] == 1
    assert len({sim[q].tobytes() for q in range(n)}) == n        # five different rows: a shifted pointer shows
    w, S, wexcl, werr = L.wcooc_ref()
    assert werr == 1 and np.isnan(w[5]).all() and (S[5] == -1).all() and wexcl[5, 0] == (1 << n) - 1
    assert np.isfinite(w[:5]).all() and (S[:5] > 0).any() and len({w[q].tobytes() for q in range(n)}) == n


def test_tsne_rows_are_past_the_cap_and_the_lattice_adds_exactly_zero():
    c, p = L.caps(), L.TSNE
    per = c["tsne_init_blocks"] * c["tsne_threads"]
    assert per == 262144 and L.passes(p["n"], per) == 2 and L.passes(p["n"] - 200, per) == 1
    assert all(iters & 1 for iters in L.TSNE_ITERS)             # odd: the init kernel copies Y into the second buffer
    Y, offsets, idx, val, rows, sub = L.tsne_case()
    assert rows.min() >= per and len(rows) == 50 and offsets[-1] == len(idx) == len(val) > 100
    assert idx.min() >= rows.min() and idx.max() <= rows.max()  # stored pairs among the 50 only
    assert (np.diff(offsets)[np.setdiff1d(np.arange(p["n"]), rows)] == 0).all()
    lat = np.delete(Y, rows, axis=0)
    assert (lat % p["spacing"] == 0).all() and lat[:, 0].min() == p["spacing"] and len(np.unique(lat, axis=0)) == len(lat)
    assert lat.max() < 2.0 ** 27 and (np.abs(Y[rows]) < 16).all()
    # the restatement itself: two lattice points beside the 50 change nothing and collect nothing
    (rx, ry, ax, ay, Z, info), (rx0, ry0, ax0, ay0, Z0, info0) = L.tsne_lattice_probe()
    assert info == info0 == 0 and Z == Z0 > 0
    for with_lattice, alone in ((rx, rx0), (ry, ry0), (ax, ax0), (ay, ay0)):
        assert np.array_equal(with_lattice[:50], alone) and (with_lattice[50:] == 0).all()
    assert (rx0 != 0).all() and (ax0 != 0).sum() > 40
    full = L.tsne_forces_ref()
    assert np.array_equal(full[0][rows], rx0) and np.count_nonzero(full[0]) == 50 and full[4] == Z0


def test_tsne_fit_reference_leaves_the_lattice_where_it_is():
    Y0, _, _, _, rows, _ = L.tsne_case()
    lattice = np.setdiff1d(np.arange(len(Y0)), rows)
    gain = 1.0
    for iters in range(1, max(L.TSNE_ITERS) + 1):
        gain = np.float64(gain) * np.float64(0.8)               # the restatement's update of a zero gradient
        if iters not in L.TSNE_ITERS:
            continue
        Y, V, G, info = L.tsne_fit_ref(iters)
        assert info == 0 and np.array_equal(Y[lattice], Y0[lattice])
        assert (V[lattice] == 0).all() and not np.signbit(V[lattice]).any() and (G[lattice] == gain).all()
        assert (Y[rows] != Y0[rows]).all() and (V[rows] != 0).all()
    assert L.tsne_fit_ref(1)[2][lattice[0], 0] == 0.8


def test_ingest_rows_are_past_the_caps():
    c = L.caps()
    assert L.passes(L.INGEST_ROWS, c["ing_minmax_blocks"] * 256) == 2
    assert L.passes(L.INGEST_ROWS, c["ing_rows_blocks"] * 256) == 1       # k_ing_anime_max / k_ing_half_filter: one pass
    assert 900 * 4 * L.INGEST_USER_SCALE > c["ing_init_blocks"] * 256     # most user ids of the frame: past k_ing_init's
    assert 3 * L.INGEST_ENCODE_IDS > c["ing_init_blocks"] * 256           # and the id bound past k_enc_init's
    assert c["ing_list_blocks"] == 4096 and L.INGEST_LIST_ROWS * 0.95 > c["ing_list_blocks"] * 256      # 1 % of the rows hold a NULL
    per = c["ing_id_max_blocks"] * c["ing_id_max_rows"]
    assert L.passes(L.ID_MAX_ROWS, per) == 2 and L.ID_MAX_ROWS - per == 7


def test_rownorm_and_boot_weights_shapes_are_past_their_caps():
    assert [L.rownorm_pass_rows(d) for d in L.ROWNORM_WIDTHS] == [131072, 16384]
    assert L.rownorm_pass_rows(L.KM_A["dim"]) < L.KM_A["n_rows"]           # the k-means tables are built past it as well
    b, per = L.BOOT_WEIGHTS, L.caps()["boot_blocks"] * 256
    assert L.passes(b["n_units"] * b["n_rep"], per) == 2 and L.passes((b["n_units"] - 1) * b["n_rep"], per) == 1


def test_flat_and_gather_shapes_are_past_their_caps():
    c = L.caps()
    assert (c["flat_blocks"], c["gather_blocks"]) == (4096, 8192)
    assert L.passes(L.FLAT_ELEMS, c["flat_blocks"] * 256) == 2 and L.FLAT_ELEMS - c["flat_blocks"] * 256 == 77
    assert L.passes(L.GATHER_ROWS, c["gather_blocks"] * 256) == 2 and L.GATHER_ROWS - c["gather_blocks"] * 256 == 33


def test_boot_sums_cover_and_ease_shapes_are_past_their_caps():
    c = L.caps()
    splits, tiles = L.boot_splits(**L.BOOT_SPLITS)
    assert (splits, tiles) == (8, 10) and L.BOOT_SPLITS["n_units"] % c["boot_tile"] != 0
    assert L.boot_splits(**dict(L.BOOT_SPLITS, n_units=splits * c["boot_tile"])) == (8, 8)       # one tile a split
    b = L.BOOT_COMBINE
    cells = (b["n_rep"] + 1) * b["n_col"]
    assert L.passes(cells, c["boot_blocks"] * 256) == 2 and L.passes(cells - b["n_col"], c["boot_blocks"] * 256) == 1
    assert L.cover_pass_items() == 6144 and L.COVER_ITEMS - L.cover_pass_items() == 9
    assert L.passes(L.EASE_ROWS, c["ease_rows"]) == 2 and L.EASE_ROWS - c["ease_rows"] == 5


def test_merge_and_scatter_shapes_are_past_their_caps():
    c = L.caps()
    assert (c["merge_blocks"], c["rec_blocks"]) == (4096, 16384)
    assert L.passes(L.MERGE_COLS, c["merge_blocks"] * 256) == 2 and L.MERGE_COLS - c["merge_blocks"] * 256 == 4099
    assert L.passes(L.SCATTER_ROWS, c["rec_blocks"] * 256) == 2 and L.SCATTER_ROWS - c["rec_blocks"] * 256 == 4099
