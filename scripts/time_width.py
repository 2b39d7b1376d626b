"""Dense train step per embedding width at the BASELINE configs[2] shape (350 000 users x 18 000 anime, batch 10 000):

    python scripts/time_width.py [--steps 200] [--rounds 4] [--out FILE]

One process, four engines alive at once — D = 32, 64, 128 and 256 — every one on the dense Adam update (lazy=False: the
lazy update exists at 128 only, so like is compared with like).  The `--steps` timed steps of each engine are taken in `--rounds` slices,
the engines alternating slice by slice, so that a drift of the box (clocks, neighbours) falls on all of them alike.
Reports ms/step (mean over the slices, and each slice) and the bytes a step moves by its shapes:
    gathers   fwd reads two rows per rating, bwd one row of the other table per contribution (2 per rating) and writes
              one chunk row per chunk (counted as one per rating: the worst case)      5 x 4D bytes per rating
    update    Adam streams W, M, V in and out                                           24 B per table element
The JSON goes to stdout (one line) and to --out."""
import json
import os
import sys
import time

os.environ["ANIREC_LAZY_ADAM"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_USERS, N_ANIME, B = 350_000, 18_000, 10_000
WARMUP = 8
CASES = (("32", 32), ("64", 64), ("128", 128), ("256", 256))


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def step_bytes(dim):
    return 5 * 4 * dim * B + 24 * (N_USERS + N_ANIME) * dim


def main():
    import torch
    import bench
    from anime_recommendations_amd.engine import TrainEngine
    steps, rounds = _arg("--steps", 200), _arg("--rounds", 4)
    per = steps // rounds
    total = WARMUP + per * rounds
    dev = torch.device("cuda:0")
    ui, ai, t = bench.synth_ratings(N_USERS, N_ANIME, total * B, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    engines = {}
    for name, dim in CASES:
        U = (torch.rand(N_USERS, dim, generator=g, device=dev) - 0.5) * 0.1
        A = (torch.rand(N_ANIME, dim, generator=g, device=dev) - 0.5) * 0.1
        eng = TrainEngine(N_USERS, N_ANIME, max_batch=B, arena_steps=64, lazy=False, width=dim)
        eng.set_head(w=1.2)
        eng.set_weights(U, A)
        eng.set_epoch(ui, ai, t, np.arange(total) * B, np.full(total, B), bench.alphas_for(total))
        eng.run(WARMUP, use_graph=True, first_step=0)
        eng.synchronize()
        engines[name] = eng
        del U, A
    slices = {name: [] for name in engines}
    for r in range(rounds):
        for name, eng in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(per, use_graph=True, first_step=WARMUP + r * per)
            eng.synchronize()
            slices[name].append((time.perf_counter() - t0) / per * 1e3)
    out = {"shape": {"users": N_USERS, "anime": N_ANIME, "batch": B, "update": "dense adam", "steps": per * rounds,
                     "rounds": rounds}, "widths": {}}
    for (name, dim), eng in zip(CASES, engines.values()):
        rec = eng.read_state()
        assert np.isfinite(rec["last_loss"]) and int(rec["step_fwd"]) == total
        ms = float(np.mean(slices[name]))
        nb = step_bytes(dim)
        out["widths"][name] = {"dim": dim, "ms_per_step": ms, "ms_per_step_slices": slices[name],
                               "bytes_per_step": nb, "gbs": nb / (ms * 1e-3) / 1e9, "loss": float(rec["last_loss"])}
        eng.close()
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
