"""Cost of the Keras-metrics path of the train step at the S109M shape (350 000 users x 18 000 anime, D = 128, batch
10 000, the default lazy Adam), default head (sigmoid + binary_crossentropy):

    python scripts/time_metrics.py [--out FILE] [--rounds R]

For the metric set ["mse"] (mask 0: the head kernel as it always was) and for the full set (every ANIREC_METRIC_* bit,
AUC included: k_head_metrics) it reports, in R interleaved rounds of one process,
  * ms/step of the graph-replayed step loop (warm-up, then 32 timed steps);
  * k_head's mean duration [us] from the in-kernel stamps (anirec_train_stage_ticks) over 8 armed eager steps.
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_metrics.py` for the k_head / k_head_metrics
kernel times.  The JSON goes to stdout (and to --out)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_USERS, N_ANIME, B = 350_000, 18_000, 10_000
WARMUP, STEPS, TICK_STEPS = 8, 32, 8
SETS = {"mse": 0, "full": 127}


def main():
    import torch
    import bench
    from anime_recommendations_amd import schedule
    from anime_recommendations_amd.engine import TrainEngine
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
    dev = torch.device("cuda:0")
    n_steps = WARMUP + STEPS + TICK_STEPS
    ui, ai, t = bench.synth_ratings(N_USERS, N_ANIME, n_steps * B, dev)
    U, A = bench.init_tables(N_USERS, N_ANIME, dev)
    engines = {}
    for name, mask in SETS.items():
        eng = TrainEngine(N_USERS, N_ANIME, max_batch=B, arena_steps=64, metrics=mask)
        eng.set_head(w=1.2)
        engines[name] = eng
    res = {name: {"ms_per_step": [], "k_head_us": []} for name in SETS}
    for _ in range(rounds):
        for name, eng in engines.items():
            eng.set_weights(U, A)
            eng.reset_optimizer()
            eng.set_epoch(ui, ai, t, np.arange(n_steps) * B, np.full(n_steps, B), schedule.adam_alphas(1e-5, 1, n_steps))
            eng.reset_metrics()
            eng.run(WARMUP, use_graph=True, first_step=0)
            eng.synchronize()
            t0 = time.perf_counter()
            eng.run(STEPS, use_graph=True, first_step=WARMUP)
            eng.synchronize()
            res[name]["ms_per_step"].append((time.perf_counter() - t0) / STEPS * 1e3)
            eng.stage_ticks(True, read=False)
            eng.run(TICK_STEPS, use_graph=False, first_step=WARMUP + STEPS)
            eng.synchronize()
            res[name]["k_head_us"].append(eng.stage_ticks(False)["head"])
    out = {"shape": [N_USERS, N_ANIME, B], "lazy": bool(engines["mse"].lazy), "rounds": rounds}
    for name in SETS:
        r = res[name]
        out[name] = {k: {"median": float(np.median(v)), "min": float(np.min(v))} for k, v in r.items()}
    out["full_logs"] = engines["full"].epoch_logs()
    for eng in engines.values():
        eng.close()
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
