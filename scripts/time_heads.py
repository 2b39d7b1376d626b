"""Per-head timing at the S109M shape (350 000 users x 18 000 anime, D = 128, batch 10 000, the default lazy update):

    python scripts/time_heads.py [--out FILE] [--pairs N]

For every (loss, activation) pair of the train step (schedule.LOSSES x schedule.ACTIVATIONS) it reports
  * ms/step of the graph-replayed step loop (warm-up, then 32 timed steps);
  * k_head's mean duration [us] from the in-kernel stamps (anirec_train_stage_ticks) over 8 armed eager steps.
For every activation it reports the predict grid on the matrix cores (100 000 users x 18 000 anime; best of 5 after a
warm-up, CUDA events) and the batched model_recs top-k (ops.predict_topk_mfma, k = 10, 100 000 users, with the exact
re-run of the rows it flags), with that fallback count.  The JSON goes to stdout (and to --out)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_USERS, N_ANIME, B = 350_000, 18_000, 10_000
WARMUP, STEPS, TICK_STEPS = 8, 32, 8
GRID_USERS = 100_000
HEADS = {"sigmoid": dict(beta=0.0), "linear": dict(beta=0.5), "tanh": dict(beta=0.0), "relu": dict(beta=0.3),
         "softplus": dict(beta=0.0)}


def time_pairs(max_pairs=None):
    import torch
    import bench
    from anime_recommendations_amd import schedule
    from anime_recommendations_amd.engine import TrainEngine
    dev = torch.device("cuda:0")
    n_steps = WARMUP + STEPS + TICK_STEPS
    ui, ai, t = bench.synth_ratings(N_USERS, N_ANIME, n_steps * B, dev)
    U, A = bench.init_tables(N_USERS, N_ANIME, dev)
    pairs = [(l, a) for l in schedule.LOSSES for a in schedule.ACTIVATIONS]
    # the default pair first and last: the spread of the two is the run-to-run noise of this process
    pairs = [("binary_crossentropy", "sigmoid")] + [p for p in pairs if p != ("binary_crossentropy", "sigmoid")]
    if max_pairs:
        pairs = pairs[:max_pairs]
    pairs.append(("binary_crossentropy", "sigmoid"))
    out = []
    for loss, act in pairs:
        eng = TrainEngine(N_USERS, N_ANIME, max_batch=B, arena_steps=64, loss=loss, activation=act)
        eng.set_head(w=1.2)
        eng.set_weights(U, A)
        eng.reset_optimizer()
        eng.set_epoch(ui, ai, t, np.arange(n_steps) * B, np.full(n_steps, B), schedule.adam_alphas(1e-5, 1, n_steps))
        eng.run(WARMUP, use_graph=True, first_step=0)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.run(STEPS, use_graph=True, first_step=WARMUP)
        eng.synchronize()
        ms = (time.perf_counter() - t0) / STEPS * 1e3
        eng.stage_ticks(True, read=False)
        eng.run(TICK_STEPS, use_graph=False, first_step=WARMUP + STEPS)
        eng.synchronize()
        ticks = eng.stage_ticks(False)
        rec = eng.read_state()
        out.append({"loss": loss, "activation": act, "lazy": bool(eng.lazy), "ms_per_step": ms,
                    "k_head_us": ticks["head"], "last_loss": float(rec["last_loss"]),
                    "finite": bool(np.isfinite(rec["last_loss"]))})
        eng.close()
        del eng
        torch.cuda.empty_cache()
    return out


def time_predict():
    import torch
    from anime_recommendations_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    U = torch.randn(GRID_USERS, 128, generator=g, device=dev) * 0.05
    A = torch.randn(N_ANIME, 128, generator=g, device=dev) * 0.05
    A[:, :4] += 0.05
    U[:, :4] += 0.05
    users = torch.arange(GRID_USERS, dtype=torch.int32, device=dev)
    out_buf = torch.empty(GRID_USERS, N_ANIME, dtype=torch.float32, device=dev)
    res = {}
    for act, extra in HEADS.items():
        head = dict(w=4.0, b=0.0, gamma=1.0, mov_mean=0.0, mov_var=1.0, activation=act, **extra)
        ops.predict_grid_mfma(U, A, head, users, out=out_buf)
        torch.cuda.synchronize()
        best = None
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.predict_grid_mfma(U, A, head, users, out=out_buf)
            e1.record()
            torch.cuda.synchronize()
            best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
        ops.predict_topk_mfma(U, A, head, users, 10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, n_fb = ops.predict_topk_mfma(U, A, head, users, 10)
        torch.cuda.synchronize()
        res[act] = {"grid_mfma_ms": best, "topk_mfma_ms": (time.perf_counter() - t0) * 1e3, "topk_fallback_rows": n_fb}
    del out_buf
    torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    mp = int(sys.argv[sys.argv.index("--pairs") + 1]) if "--pairs" in sys.argv else None
    res = {"shape": {"users": N_USERS, "anime": N_ANIME, "dim": 128, "batch": B, "update": "lazy, graph"},
           "pairs": time_pairs(mp),
           "predict": {"users": GRID_USERS, "anime": N_ANIME, "k": 10, "by_activation": time_predict()}}
    line = json.dumps(res, indent=1)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
