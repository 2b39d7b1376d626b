"""Host mirror of the reference's training driver (neural_network/neural_network.py:141-233):
``model.fit`` with LearningRateScheduler(lrfn), ModelCheckpoint(save_best_only on the monitored column) and
EarlyStopping(patience=3, restore_best_weights=True), producing the Keras ``History`` columns
``loss, <metrics>, val_loss, val_<metrics>, lr`` (``loss, mse, val_loss, val_mse, lr`` with the default metrics).
Ranking names among the metrics (``hit_rate@K``, ``ndcg@K``, ``mrr``: ``schedule.split_rank_metrics``) add one
``val_<name>`` column each, between the ``val_`` columns and ``lr``: the held-out ratings ranked every epoch
(``ops.predict_rank``, the ``evaluate`` component's definition), which ``monitor`` may name.

All arithmetic of a step runs in libanirec (HIP); this file only sequences epochs.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, ops, recs, schedule
from .data import RatingTable


@dataclass
class FitConfig:
    epochs: int = 20                 # config.yaml:68
    batch_size: int = 10_000         # config.yaml:59
    test_size: int = 10_000          # config.yaml:55
    embedding_size: int = 128        # config.yaml:63
    l2_reg_factor: float = 1e-4      # config.yaml:64
    start_lr: float = 1e-5           # implied by figure_file/anime_nn_history.csv (missing in YAML)
    min_lr: float = 1e-5
    max_lr: float = 5e-5
    rampup_epochs: int = 5
    sustain_epochs: int = 0
    exp_decay: float = 0.8
    patience: int = 3                # EarlyStopping(patience=3)  neural_network.py:198
    monitor: str = "val_loss"
    mode: str = "min"
    restore_best_weights: bool = True
    seed: int = 0                    # weight init + epoch shuffles (the reference is unseeded)
    verbose: int = 1
    use_graph: bool = True
    arena_steps: int = 64
    optimizer: str = "adam"          # config.yaml model.optimizer: adam, sgd, rmsprop, adagrad (any case)
    loss: str = "binary_crossentropy"        # config.yaml model.model_loss (schedule.LOSSES, any case / alias)
    activation: str = "sigmoid"              # config.yaml model.activation_function (schedule.ACTIVATIONS)
    kernel_initializer: str = "he_normal"    # config.yaml model.kernel_initializer (schedule.INITIALIZERS)
    metrics: tuple = ("mse",)                # config.yaml model.model_metrics (schedule.resolve_metrics), and the
                                             # ranking names hit_rate@K / ndcg@K / mrr (schedule.split_rank_metrics)
    rank_min_rating: float = 0.0             # ranking columns: the validation rows rated at or above it are the targets

    def lr(self, epoch):
        return schedule.lrfn(epoch, self.start_lr, self.max_lr, self.min_lr, self.rampup_epochs,
                             self.sustain_epochs, self.exp_decay)


@dataclass
class FitResult:
    history: dict
    U: np.ndarray
    A: np.ndarray
    head: dict
    best_U: np.ndarray = None
    best_A: np.ndarray = None
    best_head: dict = None
    best_epoch: int = -1
    stopped_epoch: int = -1
    optimizer: dict = field(default_factory=dict)
    optimizer_name: str = "adam"     # whose slots ``optimizer`` holds (weights_io.save_model's optimizer_name)
    loss: str = "binary_crossentropy"    # the head the model was trained with (canonical names)
    activation: str = "sigmoid"
    step_loop_seconds: list = field(default_factory=list)   # per epoch: wall time of the step loop alone (synchronised)
    epoch_seconds: list = field(default_factory=list)       # per epoch: shuffle + steps + metrics + validation + snapshot
    rank_seconds: list = field(default_factory=list)        # per epoch: wall time of the ranking columns (inside epoch_seconds)
    rank_baseline: dict = field(default_factory=dict)       # the ranking columns' figures of the popularity baseline


def _truncated_normal(rng, std):
    """N(0, std) cut at 2 stddev by redrawing (Keras' truncated normal)"""
    w = rng.normal(0.0, std)
    while abs(w) > 2 * std:
        w = rng.normal(0.0, std)
    return w


def init_weights(n_users, n_anime, dim=128, seed=0, initializer="he_normal"):
    """Keras initialisers at the reference's call sites: Embedding 'uniform' = U(-0.05, 0.05)
    (neural_network.py:75-85); Dense(1, kernel_initializer) with fan_in = fan_out = 1 (neural_network.py:97):
    he_normal (the default) = truncated normal, stddev sqrt(2/fan_in)/0.87962566103423978, cut at 2 stddev;
    he_uniform U(+-sqrt(6)); glorot_normal / lecun_normal the truncated normal of scale 1; glorot_uniform /
    lecun_uniform U(+-sqrt(3)); random_normal N(0, 0.05); random_uniform U(+-0.05); truncated_normal stddev 0.05
    cut at 2 stddev; zeros; ones.  Every draw comes from the one PCG64 stream, after the tables."""
    kind = schedule.resolve_initializer(initializer)
    rng = np.random.Generator(np.random.PCG64(seed))
    U = rng.uniform(-0.05, 0.05, (n_users, dim)).astype(np.float32)
    A = rng.uniform(-0.05, 0.05, (n_anime, dim)).astype(np.float32)
    fan = 1.0
    if kind in ("he_normal", "glorot_normal", "lecun_normal"):    # VarianceScaling(truncated_normal)
        scale = 2.0 if kind == "he_normal" else 1.0
        w = _truncated_normal(rng, np.sqrt(scale / fan) / 0.87962566103423978)
    elif kind in ("he_uniform", "glorot_uniform", "lecun_uniform"):   # VarianceScaling(uniform)
        lim = np.sqrt(3.0 * (2.0 if kind == "he_uniform" else 1.0) / fan)
        w = rng.uniform(-lim, lim)
    elif kind == "random_normal":
        w = rng.normal(0.0, 0.05)
    elif kind == "random_uniform":
        w = rng.uniform(-0.05, 0.05)
    elif kind == "truncated_normal":
        w = _truncated_normal(rng, 0.05)
    else:
        w = 0.0 if kind == "zeros" else 1.0
    return U, A, float(np.float32(w))


def head_of(rec):
    return {k: float(rec[k]) for k in ("w", "b", "gamma", "beta", "mov_mean", "mov_var")}


def _improved(cur, best, mode):
    return cur < best if mode == "min" else cur > best


def _column(col, rows, dtype, dev):
    """rows ``rows`` of a table column (NumPy on the host or a torch tensor already in HBM) as a device tensor"""
    col = col[rows]
    if isinstance(col, torch.Tensor):
        return col.to(device=dev, dtype=dtype).contiguous()
    np_dtype = {torch.int32: np.int32, torch.float32: np.float32}[dtype]
    return torch.as_tensor(np.asarray(col, np_dtype), device=dev)


def fit(table: RatingTable, cfg: FitConfig, engine=None, log=print, device="cuda:0") -> FitResult:
    """Train the embedding model on ``table`` (a ``data.RatingTable`` of NumPy columns or an
    ``ingest.EncodedRatings`` whose columns already live in HBM); returns History + last and best weights."""
    width = _lib.check_width(cfg.embedding_size)     # (ValueError before anything is allocated or the engine touched)
    kind = schedule.resolve_optimizer(cfg.optimizer)
    loss_name, act_name = schedule.resolve_loss(cfg.loss), schedule.resolve_activation(cfg.activation)
    point_names, rank_specs = schedule.split_rank_metrics(cfg.metrics)
    metrics = schedule.resolve_metrics(point_names, act_name)
    mask = schedule.metric_mask(metrics)
    # the default set (mse alone) reads the two sums every step keeps: epoch_metrics / evaluate, as it always did
    plain = [kind for _, kind in metrics] == ["mse"]
    keys = ["loss"] + [k for k, _ in metrics]
    rank_keys = ["val_" + key for key, _, _ in rank_specs]
    keys = keys + ["val_" + k for k in keys] + rank_keys + ["lr"]
    if cfg.monitor not in keys[:-1]:
        raise ValueError("monitor %r names no History column (%s)" % (cfg.monitor, ", ".join(keys[:-1])))
    if rank_specs:
        if engine is not None and hasattr(engine, "set_epoch_global"):
            raise ValueError("ranking metrics (%s) need the whole user table on one GPU: a multi-GPU engine shards "
                             "the user rows (rank a saved model with the evaluate component)"
                             % ", ".join(key for key, _, _ in rank_specs))
        r_users, r_row, r_anime, _ = recs.held_out_targets(table, cfg.test_size, cfg.rank_min_rating)
        if len(r_row) == 0:
            raise ValueError("no validation row is rated at or above rank_min_rating = %r: the ranking metrics (%s) "
                             "have no target" % (cfg.rank_min_rating, ", ".join(key for key, _, _ in rank_specs)))
        rank_ks = sorted({k for _, _, k in rank_specs if k is not None})
    tr, te = table.split(cfg.test_size)
    n_train = tr.stop - tr.start
    if engine is None:
        from .engine import TrainEngine
        engine = TrainEngine(table.n_users, table.n_anime, max_batch=min(cfg.batch_size, n_train),
                             l2=cfg.l2_reg_factor, arena_steps=cfg.arena_steps, device=device, optimizer=kind,
                             loss=loss_name, activation=act_name, metrics=mask, width=width)
    elif getattr(engine, "optimizer", "adam") != kind:
        raise ValueError("the engine was built for optimizer %r, the config asks for %r"
                         % (getattr(engine, "optimizer", "adam"), kind))
    for what, want, default in (("loss", loss_name, "binary_crossentropy"), ("activation", act_name, "sigmoid")):
        have = getattr(engine, what, default)
        if have != want:
            raise ValueError("the engine was built for %s %r, the config asks for %r" % (what, have, want))
    if getattr(engine, "width", _lib.DIM) != width:
        raise ValueError("the engine was built for embedding width %d, the config asks for %d"
                         % (getattr(engine, "width", _lib.DIM), width))
    if getattr(engine, "metrics", 0) != mask:
        raise ValueError("the engine accumulates metrics %#x, the config asks for %#x (%s)"
                         % (getattr(engine, "metrics", 0), mask, ", ".join(k for k, _ in metrics)))
    dev = engine.device
    U0, A0, w0 = init_weights(table.n_users, table.n_anime, width, cfg.seed, cfg.kernel_initializer)
    engine.set_head(w=w0)
    engine.set_weights(U0, A0)
    engine.reset_optimizer()

    ui, ai, rt = (_column(c, tr, dt, dev) for c, dt in ((table.user, torch.int32), (table.anime, torch.int32),
                                                        (table.rating, torch.float32)))
    vu, va, vt = (_column(c, te, dt, dev) for c, dt in ((table.user, torch.int32), (table.anime, torch.int32),
                                                        (table.rating, torch.float32)))

    B = min(cfg.batch_size, n_train)
    # multi-GPU (dist.DistTrainEngine): each rank takes B ratings of a global batch of G*B
    Bg = int(getattr(engine, "global_batch", B))
    starts = np.arange(0, n_train, Bg)
    counts = np.minimum(Bg, n_train - starts)
    n_steps = len(starts)
    multi = hasattr(engine, "set_epoch_global")
    gen = torch.Generator(device=dev)
    hist = {k: [] for k in keys}
    best = np.inf if cfg.mode == "min" else -np.inf
    best_w = None
    best_epoch, stopped, wait = -1, -1, 0
    t_global = 0
    loop_s, epoch_s, rank_s = [], [], []
    rank_baseline = {}
    if rank_specs:
        # once: the targets, the watched bits of the listed users alone and the popularity baseline on the same targets
        with torch.cuda.device(dev):
            r_row_t, r_anime_t = (torch.as_tensor(x, device=dev).to(torch.int32) for x in (r_row, r_anime))
            r_users_t = torch.as_tensor(r_users, device=dev).to(torch.int32)
            r_bits = recs.listed_seen_bits(ui, ai, r_users, table.n_users, table.n_anime, device=dev)
            score = recs.popularity_scores(ai, table.n_anime, table.n_users)
            base = recs.ranking_metrics(ops.score_rank(score, len(r_users), r_row_t, r_anime_t, watched_bits=r_bits),
                                        rank_ks)
        rank_baseline = {"val_" + k: v for k, v in recs.rank_figures(base, rank_specs).items()}
        log("Popularity baseline on the %d ranking targets of %d users - %s"
            % (len(r_row), len(r_users), " - ".join("%s: %.4f" % kv for kv in rank_baseline.items())))
    for epoch in range(cfg.epochs):
        t_epoch = time.perf_counter()
        lr = cfg.lr(epoch)
        gen.manual_seed(cfg.seed * 1_000_003 + epoch)
        perm = torch.randperm(n_train, generator=gen, device=dev)     # model.fit(shuffle=True)
        alphas = schedule.step_rates(kind, lr, t_global + 1, n_steps)
        if multi:
            import torch.distributed as dist
            if dist.is_initialized() and dist.get_world_size() > 1:
                dist.broadcast(perm, src=0)                           # one shuffle for all ranks
            engine.set_epoch_global(ui, ai, rt, perm, alphas)
        else:
            eu, ea, et = ops.gather_ratings(ui, ai, rt, perm)
            engine.set_epoch(eu, ea, et, starts, counts, alphas)
        engine.reset_metrics()
        engine.synchronize()
        t_loop = time.perf_counter()
        engine.run(n_steps, use_graph=cfg.use_graph)
        engine.synchronize()
        loop_s.append(time.perf_counter() - t_loop)
        t_global += n_steps
        if plain:
            loss, mse = engine.epoch_metrics()
            val_loss, val_mse = engine.evaluate(vu, va, vt)
            logs, val_logs = {"loss": loss, "mse": mse}, {"loss": val_loss, "mse": val_mse}
        else:
            logs, val_logs = engine.epoch_logs(), engine.eval_logs(vu, va, vt)
        row = [logs["loss"]] + [logs[kind] for _, kind in metrics]
        row += [val_logs["loss"]] + [val_logs[kind] for _, kind in metrics]
        if rank_specs:
            # the tables are current here, as for the snapshot below: the engine's stream is drained, the rank kernels
            # run on torch's and are finished (the ranks are read back) before the next epoch writes W
            t_rank = time.perf_counter()
            engine.synchronize()
            with torch.cuda.device(dev):
                rank, _ = ops.predict_rank(engine.U, engine.A, dict(head_of(engine.read_state()), activation=act_name),
                                           r_users_t, r_row_t, r_anime_t, watched_bits=r_bits)
                row += list(recs.rank_figures(recs.ranking_metrics(rank, rank_ks), rank_specs).values())
                torch.cuda.synchronize(dev)
            rank_s.append(time.perf_counter() - t_rank)
        row.append(float(np.float32(lr)))
        for k, v in zip(keys, row):
            hist[k].append(v)
        if cfg.verbose:
            log("Epoch %d/%d - %s - lr: %.4g" % (epoch + 1, cfg.epochs,
                                                 " - ".join("%s: %.4f" % (k, v) for k, v in zip(keys, row[:-1])), lr))
        cur = hist[cfg.monitor][-1]
        if _improved(cur, best, cfg.mode):                             # ModelCheckpoint / best_weights
            best, best_epoch, wait = cur, epoch, 0
            # snapshot on the device (a 188 MB table copies in ~0.1 ms there, ~60 ms through the host);
            # it is brought to the host once, after the last epoch
            engine.synchronize()
            best_w = (engine.U.clone(), engine.A.clone(), head_of(engine.read_state()))
            if torch.device(dev).type == "cuda":
                torch.cuda.synchronize(dev)   # the clones ran on torch's stream: finish before the next epoch writes W
        else:
            wait += 1
        engine.synchronize()
        epoch_s.append(time.perf_counter() - t_epoch)
        if wait >= cfg.patience and epoch > 0:                        # EarlyStopping
            stopped = epoch
            break
    engine.synchronize()
    rec = engine.read_state()
    res = FitResult(history=hist, U=engine.U.cpu().numpy().copy(), A=engine.A.cpu().numpy().copy(),
                    head=head_of(rec), best_epoch=best_epoch, stopped_epoch=stopped, step_loop_seconds=loop_s,
                    epoch_seconds=epoch_s, optimizer_name=kind, loss=loss_name, activation=act_name,
                    rank_seconds=rank_s, rank_baseline=rank_baseline)
    if hasattr(engine, "optimizer_state"):       # optimiser slots and the step count of the LAST epoch (model.save)
        res.optimizer = engine.optimizer_state(iterations=t_global)
    if best_w is not None:
        best_w = (best_w[0].cpu().numpy(), best_w[1].cpu().numpy(), best_w[2])
        res.best_U, res.best_A, res.best_head = best_w
        if stopped >= 0 and cfg.restore_best_weights:
            res.U, res.A, res.head = best_w
    return res


def history_frame(history):
    """pandas frame with the reference's History CSV layout: `,loss,<metrics>,val_loss,val_<metrics>,lr`
    (`,loss,mse,val_loss,val_mse,lr` with the default metrics), the columns in ``fit``'s order."""
    import pandas as pd
    keys = [k for k in history if k != "lr"] + (["lr"] if "lr" in history else [])
    return pd.DataFrame({k: history[k] for k in keys})
