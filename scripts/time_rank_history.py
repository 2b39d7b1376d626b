"""trainer.fit's epoch loop at the 7 M-rating synthetic shape (15 000 users x 17 560 anime, D = 128, 10 000 held-out
rows) with or without the ranking columns: `time_rank_history.py plain|rank [epochs]`, one mode per process.  Prints
one JSON line: epoch_seconds, step_loop_seconds and, with the ranking names, rank_seconds (the per-epoch
ops.predict_rank + host metrics, inside epoch_seconds), the number of targets and the popularity baseline."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anime_recommendations_amd import data, recs, trainer  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "rank"
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
assert mode in ("plain", "rank")
table = data.encode_frame(data.synth_user_stats(n_users=15_000, n_anime=17_560, n_ratings=7_000_000))
metrics = ("mse",) if mode == "plain" else ("mse", "hit_rate@10", "ndcg@10", "mrr")
cfg = trainer.FitConfig(epochs=epochs, batch_size=10_000, test_size=10_000, verbose=0, patience=epochs + 1,
                        metrics=metrics, rank_min_rating=0.7)
t0 = time.perf_counter()
res = trainer.fit(table, cfg)
total = time.perf_counter() - t0
out = {"device": torch.cuda.get_device_name(0), "mode": mode, "ratings": len(table), "epochs": epochs,
       "fit_seconds": total, "epoch_seconds": [round(x, 4) for x in res.epoch_seconds],
       "step_loop_seconds": [round(x, 4) for x in res.step_loop_seconds]}
if mode == "rank":
    users, row, _, _ = recs.held_out_targets(table, cfg.test_size, cfg.rank_min_rating)
    out.update({"rank_seconds": [round(x, 5) for x in res.rank_seconds], "targets": len(row), "listed_users": len(users),
                "rank_baseline": res.rank_baseline,
                "last_epoch": {k: v[-1] for k, v in res.history.items() if k.startswith("val_")}})
print(json.dumps(out))
