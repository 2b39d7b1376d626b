"""Per-kind timing of the dense optimiser step at the S109M shape (350 000 users x 18 000 anime, D = 128, batch 10 000,
dense update for every kind — Adam included, so the four kernels are compared on the same path):

    python scripts/time_optimizers.py [--out FILE]     # ms/step per kind + the update kernel under rocprofv3

For each of adam, sgd, rmsprop and adagrad it reports
  * ms/step of the graph-replayed step loop (warm-up, then 32 timed steps);
  * the update kernel's mean duration from a SEPARATE `rocprofv3 --kernel-trace --stats` run of this script
    (`--steps-only`: a few eager steps of every kind, nothing timed in-process), and that time's share of 8 TB/s on
    the kernel's algorithmic table bytes: Adam 24 B/element (W, M, V read + written), RMSprop / Adagrad 16 (W, V),
    SGD 8 (W).  The chunk sums and the row map add about 12 MB per step, not counted.
The JSON goes to stdout (and to --out)."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

KINDS = ("adam", "sgd", "rmsprop", "adagrad")
BYTES_PER_ELEM = {"adam": 24, "sgd": 8, "rmsprop": 16, "adagrad": 16}
KERNEL = {"adam": "k_adam<true, 0, 128>", "sgd": "k_adam<true, 1, 128>", "rmsprop": "k_adam<true, 2, 128>",
          "adagrad": "k_adam<true, 3, 128>"}      # k_adam<kNT, kOpt (ANIREC_OPT_*), kD>
HBM_BPS = 8e12
N_USERS, N_ANIME, B = 350_000, 18_000, 10_000
WARMUP, STEPS = 8, 32


def _engine(kind, dev, n_steps):
    import bench
    from anime_recommendations_amd import schedule
    from anime_recommendations_amd.engine import TrainEngine
    ui, ai, t = bench.synth_ratings(N_USERS, N_ANIME, n_steps * B, dev)
    U, A = bench.init_tables(N_USERS, N_ANIME, dev)
    eng = TrainEngine(N_USERS, N_ANIME, max_batch=B, arena_steps=64, lazy=False, optimizer=kind)
    eng.set_head(w=1.2)
    eng.set_weights(U, A)
    eng.reset_optimizer()
    eng.set_epoch(ui, ai, t, np.arange(n_steps) * B, np.full(n_steps, B), schedule.step_rates(kind, 1e-5, 1, n_steps))
    return eng


def time_steps():
    import torch
    dev = torch.device("cuda:0")
    out = {}
    for kind in KINDS:
        eng = _engine(kind, dev, WARMUP + STEPS)
        eng.run(WARMUP, use_graph=True, first_step=0)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.run(STEPS, use_graph=True, first_step=WARMUP)
        eng.synchronize()
        dt = time.perf_counter() - t0
        rec = eng.read_state()
        assert np.isfinite(rec["last_loss"]) and int(rec["step_fwd"]) == WARMUP + STEPS
        out[kind] = {"ms_per_step": dt / STEPS * 1e3, "loss": float(rec["last_loss"])}
        eng.close()
        del eng
        torch.cuda.empty_cache()
    return out


def steps_only():
    """The profiled child: 12 eager steps of every kind.  The stats are per kernel name, so each kind's update kernel
    gets its own row."""
    import torch
    dev = torch.device("cuda:0")
    for kind in KINDS:
        eng = _engine(kind, dev, 12)
        eng.run(12, use_graph=False, first_step=0)
        eng.synchronize()
        eng.close()
        del eng
        torch.cuda.empty_cache()


def kernel_stats(timeout_s=900):
    d = tempfile.mkdtemp(prefix="time_optimizers_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "opt", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--steps-only"]
    subprocess.run(cmd, check=True, timeout=timeout_s, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % d)
    rows = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Name"].replace("void ", "").replace("anirec::", "").split("(")[0]
        rows[name] = r
    elems = (N_USERS + N_ANIME) * 128
    out = {}
    for kind in KINDS:
        r = rows.get(KERNEL[kind])
        if r is None:
            out[kind] = None
            continue
        us = float(r["AverageNs"]) / 1e3
        nbytes = BYTES_PER_ELEM[kind] * elems
        out[kind] = {"kernel": KERNEL[kind], "calls": int(r["Calls"]), "avg_us": us, "min_us": float(r["MinNs"]) / 1e3,
                     "algorithmic_bytes": nbytes, "floor_us_at_8tbs": nbytes / HBM_BPS * 1e6,
                     "frac_of_8tbs": nbytes / (us * 1e-6) / HBM_BPS}
    return out


if __name__ == "__main__":
    if "--steps-only" in sys.argv:
        steps_only()
        sys.exit(0)
    res = {"shape": {"users": N_USERS, "anime": N_ANIME, "dim": 128, "batch": B, "update": "dense"},
           "steps": time_steps(), "update_kernel": kernel_stats()}
    line = json.dumps(res, indent=1)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
