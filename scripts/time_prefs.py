"""All-users favourite profile (anirec_fave_profile) at 350 000 users x 17 560 anime, on the favourites of the
synthetic 109 M-rating table bench.run_user_recs builds; 43 genre-like categories, 1-4 per anime, one of them on
60 % of the anime.  Prints one JSON line: time per call and the fraction of the HBM peak.  Run under
`rocprofv3 --kernel-trace --stats` for the kernel time."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from anime_recommendations_amd import recs  # noqa: E402

n_users, n_anime, n, n_cat = 350_000, 17_560, 109_000_000, int(sys.argv[1]) if len(sys.argv) > 1 else 43
dev = torch.device("cuda")
ui, ai, t = bench.synth_ratings(n_users, n_anime, n, dev)
order = torch.sort(ui, stable=True)[1]
ui, ai, r = ui[order], ai[order], t[order].double()
del order, t
fav, _ = recs.user_favourites(ui, ai, r, n_users, n_anime)
del ui, ai, r
torch.cuda.synchronize()
rng = np.random.default_rng(5)
cat = np.zeros((n_anime, (n_cat + 31) // 32), np.uint32)
for a in range(n_anime):
    cs = set(rng.choice(n_cat, int(rng.integers(1, 5)), replace=False).tolist())
    if rng.random() < 0.6:
        cs.add(0)
    for c in cs:
        cat[a, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
cat_t = torch.from_numpy(cat.view(np.int32)).to(dev)
for _ in range(3):
    counts = recs.fave_profile(fav, cat_t, n_cat)
torch.cuda.synchronize()
reps = 20
t0 = time.perf_counter()
for _ in range(reps):
    counts = recs.fave_profile(fav, cat_t, n_cat)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / reps
ww = (n_anime + 31) // 32
nbytes = n_users * ww * 4 + n_users * n_cat * 4 + cat.nbytes     # bit rows read once, counts written once
print(json.dumps({"kernel": "k_fave_profile<%d>" % ((n_cat + 31) // 32), "n_users": n_users, "n_anime": n_anime,
                  "n_cat": n_cat, "ms_per_call_incl_host": dt * 1e3, "bytes": nbytes,
                  "gbs_incl_host": nbytes / dt / 1e9, "hbm_frac_incl_host": nbytes / dt / 1e9 / bench.HBM_PEAK_GBS,
                  "mean_favourites_per_user": float(np.unpackbits(fav[:2000].cpu().numpy().view(np.uint8)).sum()
                                                    / 2000)}))
